"""Fusion passes: rewrite TF op chains into fused ops backed by gfx950 kernels.

Patterns (matched on the constant-folded IR, only when every intermediate has
a single consumer and is not fetched):

* ``[Pad] -> Conv2D -> [BiasAdd] -> [FusedBatchNorm*] -> [Add(residual)] -> [Relu]``
  => ``_FusedConv2D``: BN folded into the weights at load time (w' = w*gamma/
  sqrt(var+eps), b' = beta - mean*scale), spatial Pad absorbed into the conv's
  explicit padding, residual add + ReLU in the MFMA kernel's epilogue.  A conv
  whose input has C % 8 != 0 (the RGB stem) reads the fp32 request tensor
  directly (ingest cast fused into the operand loads).
* ``Mul(Relu6(Add(x, 3)), 1/6)`` => ``_HardSigmoid(x)``; ``Mul(x, _HardSigmoid(x))`` (or
  the slim association ``Mul(Mul(x, Relu6(Add(x, 3))), 1/6)``) => ``_HardSwish(x)``, which
  ``_FusedConv2D`` / ``_FusedDepthwiseConv2D`` take as their closing activation
  (MobileNetV3; igemm and dwconv epilogues).
* ``Mul(x, _HardSigmoid(Conv2D 1x1(act(Conv2D 1x1(_GlobalAvgPool(x))))))`` =>
  ``_SqueezeExcite(x)``: fp32 FC weights, ``se_gate`` + ``se_scale`` (kernels/se.hip).
* ``Mul(x, Sigmoid(x))``, ``Mul(x, Sigmoid(Mul(x, 1.0)))`` and either one behind output 0 of
  the ``custom_gradient`` ``IdentityN`` => ``_Swish(x)``, a closing activation like
  ``_HardSwish`` (EfficientNet); the squeeze-excite pattern with a ``Sigmoid`` gate and a none /
  ``Relu`` / ``_Swish`` inner activation => ``_SqueezeExciteSigmoid(x)``.
* ``[Pad] -> DepthwiseConv2dNative -> [BiasAdd] -> [FusedBatchNorm*] -> [Relu|Relu6|_HardSwish|_Swish]``
  => ``_FusedDepthwiseConv2D`` (channel multiplier 1): BN folded into the fp32
  filter, one ``dwconv2d`` launch (kernels/dwconv.hip).  ``Relu6`` also fuses
  into ``_FusedConv2D`` (MobileNet's pointwise convs).
* ``_LayerNorm(_FusedDepthwiseConv2D(x))`` with a 7x7 / stride-1 depthwise op without
  activation => ``_FusedDepthwiseLN`` (ConvNeXt): one ``dwconv_ln`` launch
  (kernels/dwln.hip), the conv result in fp32 up to the normalised output's one
  rounding.  A tanh / erf GELU subgraph closes a ``_FusedConv2D`` chain like a
  one-node activation (after the residual add), and ConvNeXt's layer scale and
  shortcut are the chain's ``Mul`` by a ``[C]`` constant and residual ``AddV2``.
* ``[Pad] -> Conv2D -> [BiasAdd] -> [FusedBatchNorm*] -> [Relu]`` whose input has a
  known multiple of the filter's in-depth channels (a grouped conv: ResNeXt)
  => ``_FusedGroupedConv2D``: BN folded, one ``gconv2d`` launch (kernels/gconv.hip)
  for 3x3 filters with 4 / 8 / 16 / 32 channels per group.
  (The dense, depthwise and grouped patterns share their head, ``[Pad] -> conv ->
  [BiasAdd] -> [FusedBatchNorm*]`` and its guards: ``_match_conv_chain``.)
* ``MatMul -> [BiasAdd] -> [Add(residual)] -> [Relu|Tanh|GELU]`` => ``_FusedMatMul``
  (fp32 output when it feeds a Softmax/ArgMax head or is fetched).
* ``Mean(NHWC, axes=[1,2])`` => ``_GlobalAvgPool``;  ``MaxPool`` => ``_MaxPool``;
  the ResNet stem ``_FusedConv2D(7x7/2, RGB) -> _MaxPool(3x3/2)`` => ``_StemPool``.
* ``Softmax(x)`` + ``ArgMax(x, -1)`` on the same logits => ``_SoftmaxArgMax``.
* ViT: ``AddV2(ConcatV2([Tile|BroadcastTo(cls, [batch, ..]), Reshape(x, [-1, P, C])], 1), pos)``
  => ``_PatchTokens(x, batch)``: class token, patches and position embedding in one
  ``patch_tokens`` launch (kernels/misc.hip) from an fp32 ``[P + 1, C]`` table.
* DLRM (``graph/patterns.py``): ``Pack([x0?, Sum(GatherV2(table_f, ids_f, 0), 1) ..], 1)`` =>
  ``_EmbeddingBag`` (kernels/embag.hip); ``[Pad(] ConcatV2([dense, GatherV2(Reshape(BatchMatMul(Z, Z,
  adj_y), [-1, F F]), tril idx, 1)], 1) [)]`` => ``_DotInteraction`` (kernels/interact.hip).
* BERT: decomposed LayerNorm => ``_LayerNorm``; tanh/erf GELU subgraphs => act
  of the producing ``_FusedMatMul``; Q/K/V projections + attention core =>
  ``_FusedQKV`` + ``_Attention`` (see ``bert_passes``); Swin's windowed attention as
  ``_FusedQKV`` + ``_WindowAttention`` with the window layout folded into the op.

On a CUDA/HIP device the fused ops launch the ``_hip`` kernels (bf16 operands,
fp32 accumulate); on the CPU they run an fp32 torch reference of the *same*
folded parameters, which is how the passes are validated without a GPU.
"""
from __future__ import annotations

import os
from typing import Dict, List, Optional, Sequence, Set, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from ..utils import tensors as T
from . import ops as O
from .ir import Graph, Node
from .placement import to_device, zeros

BF16 = torch.bfloat16
IGEMM_ONLY_ACTS = ("relu6", "hard_swish", "swish")    # ops.IGEMM_ONLY_ACTS: no cgemm / bgemm / halo epilogue
# the ops fuse_conv / fuse_depthwise take as the closing activation -> the kernels' name for it
_CLOSING_ACTS = {"Relu": "relu", "Relu6": "relu6", "_HardSwish": "hard_swish", "_Swish": "swish"}


# ------------------------------------------------------------------ helpers
def _const(g: Graph, ref) -> Optional[torch.Tensor]:
    n = g.nodes.get(ref[0])
    if n is None or n.op != "Const" or n.value is None:
        return None
    v = n.value[ref[1]] if ref[1] < len(n.value) else None
    return v if isinstance(v, torch.Tensor) else None


def _channel_const(v: Optional[torch.Tensor], c: int, rank: int) -> Optional[torch.Tensor]:
    """``v`` as a flat fp32 [c] vector (or a one-element tensor) when it
    broadcasts along the LAST axis of a rank-``rank`` tensor with ``c``
    channels and nowhere else: its shape, leading 1s dropped, is ``(c,)``, or
    it has one element; and it has no more axes than the tensor (a longer
    shape would raise the result's rank).  A size check alone is not enough: a
    ``[c, 1]`` constant has ``c`` elements and scales along W, not along C."""
    if v is None or v.dim() > rank:
        return None
    if v.numel() == 1:
        return v.float().reshape(1)
    shape = list(v.shape)
    while shape and shape[0] == 1:
        shape.pop(0)
    return v.float().reshape(-1) if shape == [c] else None


def _residual_for(res: torch.Tensor, out_shape) -> Optional[torch.Tensor]:
    """The residual as the kernels read it (one element per output element):
    itself, its broadcast to the output's shape, or None when adding it would
    change the output's shape (the op then adds it with torch)."""
    out_shape = tuple(out_shape)
    if tuple(res.shape) == out_shape:
        return res
    try:
        if tuple(torch.broadcast_shapes(tuple(res.shape), out_shape)) != out_shape:
            return None
    except RuntimeError:
        return None
    return res.expand(out_shape)


def _add_residual_unfused(impl, ctx, node, x, res):
    """``act(op(x) + res)`` for a residual the kernels cannot take: the op
    without its residual, activation and post output, then torch."""
    plain = impl.__class__.__new__(impl.__class__)
    plain.__dict__.update(impl.__dict__)
    plain.act, plain.post, plain.post_mode = "none", None, None
    y = plain(ctx, node, [x])[0]
    z = _ref_act(y.float() + res.float().to(y.device), impl.act)
    z = z.to(y.dtype) if y.dtype == BF16 else z
    if getattr(impl, "post", None) is None:
        return [z.contiguous()]
    return [o.to(y.dtype) for o in _with_post(impl, z.contiguous())]     # (the kernels' post output is bf16 too)


class _Ctx:
    def __init__(self, g: Graph, order: List[str], fed: Set[str], fetch_refs, device, opts):
        self.g = g
        self.order = order
        self.fed = fed
        self.fetch_nodes = {n for n, _ in fetch_refs}
        self.fetch_refs = set(fetch_refs)
        self.device = device
        self.opts = opts
        self.use_hip = device.type == "cuda"
        self.cons = g.consumers()

    def only_consumer(self, name: str, idx: int = 0) -> Optional[Node]:
        """The unique consumer of output ``idx`` of ``name`` (and no other output used)."""
        if name in self.fetch_nodes:
            return None
        cs = self.cons.get(name, [])
        if len(cs) != 1:
            return None
        cname, _pos, oidx = cs[0]
        if oidx != idx:
            return None
        return self.g.nodes[cname]

    def refresh(self):
        self.cons = self.g.consumers()


def _merge_ctrl(nodes: Sequence[Node]) -> List[str]:
    out: List[str] = []
    names = {n.name for n in nodes}
    for n in nodes:
        for c in n.ctrl:
            if c not in out and c not in names:
                out.append(c)
    return out


def _finalize(g: Graph, chain: List[Node], op: str, inputs, attrs) -> Node:
    last = chain[-1]
    ctrl = _merge_ctrl(chain)
    for n in chain[:-1]:
        del g.nodes[n.name]
    last.op = op
    last.inputs = list(inputs)
    last.ctrl = ctrl
    last.attrs = attrs
    last.value = None
    return last


def _pad_k(w_nk: torch.Tensor, mult: int = 64) -> torch.Tensor:
    n, k = w_nk.shape
    kp = -(-k // mult) * mult
    if kp != k:
        w_nk = torch.cat([w_nk, torch.zeros(n, kp - k, dtype=w_nk.dtype, device=w_nk.device)], dim=1)
    return w_nk


def _to_bf16(x: torch.Tensor) -> torch.Tensor:
    if x.dtype == BF16:
        return x
    if x.dtype == torch.float32 and x.is_cuda and x.is_contiguous():
        from ..ops import hip
        return hip().cast_bf16(x)
    return x.to(BF16).contiguous()


# ------------------------------------------------------------------ fused op impls
class _Window:
    """The kh x kw window, stride (sh, sw), that the conv and pool ops slide over
    H and W of an NHWC tensor.  Methods and plain fields only: the tensors of an
    op are its own (placement.weight_refs lays them out by attribute name)."""

    def _set_window(self, kh: int, kw: int, strides, padding: str, pads):
        self.kh, self.kw = kh, kw
        self.sh, self.sw = strides
        self.padding = padding          # "SAME" | "VALID" | "EXPLICIT"
        self.pads = pads                # (pt, pb, pl, pr) for EXPLICIT

    def pads_for(self, h, w):
        if self.padding == "SAME":
            return O.tf_same_pads(h, self.kh, self.sh) + O.tf_same_pads(w, self.kw, self.sw)
        if self.padding == "EXPLICIT":
            return tuple(self.pads)
        return (0, 0, 0, 0)

    def out_hw(self, h, w, pads, kh=None, kw=None):
        """(ho, wo) of an h x w input under ``pads``; ``kh`` / ``kw`` stand in
        for the window's own extent (FusedConv's padded RGBA filter)."""
        pt, pb, pl, pr = pads
        kh, kw = self.kh if kh is None else kh, self.kw if kw is None else kw
        return (h + pt + pb - kh) // self.sh + 1, (w + pl + pr - kw) // self.sw + 1


def _grouped_conv_torch(x: torch.Tensor, w_hwio: torch.Tensor, bias: torch.Tensor, strides, pads, groups: int):
    """NHWC ``conv2d(pad(x), w, groups=) + bias`` in the dtype of ``x`` (the
    interpreter's Conv2D, ops._conv2d: the same calls, so the same errors).
    The one reference conv of the fused ops: dense is ``groups`` 1, depthwise
    ``groups`` C with the filter as [kh, kw, 1, C]."""
    pt, pb, pl, pr = pads
    xc = x.permute(0, 3, 1, 2)
    xc = F.pad(xc, [pl, pr, pt, pb]) if (pt or pb or pl or pr) else xc
    y = F.conv2d(xc, w_hwio.to(x.dtype).permute(3, 2, 0, 1), stride=tuple(strides), groups=groups)
    return y.permute(0, 2, 3, 1) + bias.to(x.dtype)


# The row-panel kernel (kernels/panel.hip) as further options of a wide 1x1
# conv; TFSERVE_PANEL=0 (read once) removes them (A/B in one build).
_PANEL = os.environ.get("TFSERVE_PANEL", "1") != "0"


def panel_eligible(kh, kw, sh, sw, pads, cin, cout, act, post=None, c4=False) -> bool:
    """A conv the row-panel kernel may take: 1x1, stride 1, unpadded, ``cin``
    one of the kernel's depths, at least twice as wide as deep (a bottleneck's
    expand conv: the wider the output, the more re-reads of A the panel saves),
    act none / relu, no post-activation output.  (bf16 NHWC input: every conv
    with ``cin % 8 == 0`` has it.)"""
    return (kh == 1 and kw == 1 and sh == 1 and sw == 1 and not any(pads) and cin in (128, 256, 512) and
            cout % 64 == 0 and cout >= 2 * cin and act in ("none", "relu") and post is None and not c4)


def panel_key(x_shape, cout, has_res, act):
    """The ``ops.tuned_choice`` key of a panel-eligible conv: option 0 = the
    tile-config path, i = the i-th form of ``hip().conv1x1_panel_forms``.  A
    key kind of its own, timed at load: not part of the committed table."""
    return ("panel", tuple(x_shape), cout, bool(has_res), act)


class FusedConv(_Window):
    """Conv2D(+folded BN/bias)(+residual)(+act).  Weights: HWIO fp32 (reference)
    and [Cout][Kpad] bf16 (kernel)."""

    def __init__(self, w_hwio: torch.Tensor, bias: torch.Tensor, strides, padding: str, pads, act: str,
                 device: torch.device, use_hip: bool, name: str):
        kh, kw, self.cin, self.cout = w_hwio.shape
        self._set_window(kh, kw, strides, padding, pads)
        self.act = act
        self.use_hip = use_hip
        self.name = name
        self.device = device
        # RGB(A) stems: the fp32 request is re-laid out as zero-bordered bf16 RGBA
        # (ingest_c4_padded), weights as [Cout][kh (padded to even)][8 taps][4 ch]:
        # a 64-deep k-tile is then 2 filter rows x 8 taps x 4 channels = two
        # contiguous 64-B runs of the padded image, DMA'd with no bounds checks
        self.c4 = use_hip and self.cin <= 4 and self.kw <= 8
        self.khp = self.kh + (self.kh % 2) if self.c4 else self.kh
        if use_hip:
            if self.c4:
                w4 = torch.zeros(self.khp, 8, 4, self.cout, device=w_hwio.device)
                w4[:self.kh, :self.kw, :self.cin, :] = w_hwio.float()
                w_nk = w4.permute(3, 0, 1, 2).reshape(self.cout, self.khp * 32)
            else:
                k = self.kh * self.kw * self.cin
                w_nk = w_hwio.permute(3, 0, 1, 2).reshape(self.cout, k)
            self.w = to_device(_pad_k(w_nk).to(BF16), device)
            self.b = to_device(bias.float(), device)
        else:
            self.w_ref = to_device(w_hwio.float(), device)
            self.b_ref = to_device(bias.float(), device)

    # ---- post-activation output (ResNet v2 pre-activation of the next block)
    post = None          # (scale [Cout], shift [Cout], act) on the device / CPU
    post_mode = None     # "dual": [raw, post]; "only": [post]

    def set_post(self, scale: torch.Tensor, shift: torch.Tensor, act: str, mode: str):
        dev = self.device if self.use_hip else (self.w_ref.device if hasattr(self, "w_ref") else "cpu")
        self.post = (to_device(scale.float(), dev), to_device(shift.float(), dev), act)
        self.post_mode = mode

    def post_ok(self) -> bool:
        """The fused kernels write the post output only on the cgemm / halo
        paths (64-aligned channels); the CPU reference always can."""
        return not self.use_hip or (not self.c4 and self.cin % 64 == 0 and self.cout % 8 == 0 and
                                    self.act not in IGEMM_ONLY_ACTS)   # (the post output is cgemm / halo only; they
        #                                                                  have no relu6 / hard_swish)

    def _hwio(self) -> torch.Tensor:
        """The folded filter as fp32 HWIO, from whichever form this op keeps."""
        if not self.use_hip:
            return self.w_ref
        if self.c4:
            w = self.w[:, :self.khp * 32].reshape(self.cout, self.khp, 8, 4)[:, :self.kh, :self.kw, :self.cin]
        else:
            w = self.w[:, :self.kh * self.kw * self.cin].reshape(self.cout, self.kh, self.kw, self.cin)
        return w.float().permute(1, 2, 3, 0)

    def _torch(self, x, res, pads):
        """The fp32 reference (the CPU path), and on the device an input with
        another channel count than the filter's in-depth (the pass could not
        see it): Conv2D's own semantics with torch -- a grouped conv when the
        counts divide, else torch's error, which the executor reports as the
        interpreter's Conv2D does."""
        w = self._hwio().to(x.device)
        b = (self.b if self.use_hip else self.b_ref).to(x.device)
        y = _grouped_conv_torch(x.float(), w, b, (self.sh, self.sw), pads, x.shape[3] // self.cin)
        if res is not None:
            y = y + res.float()
        outs = _with_post(self, _ref_act(y, self.act).contiguous())
        return [o.to(BF16) for o in outs] if self.use_hip else outs

    def panel_choice(self, ctx, node, ins) -> Optional[int]:
        """The tuned choice between the tile-config path (0) and the row-panel
        kernel's forms (1, 2, ...) for these inputs, made without a launch
        unless it has to be timed; None when the conv is not offered to that
        kernel.  ``ChainConv`` asks before its own choice, so the chain is timed
        against the expand conv's best form as a separate launch."""
        x = O.to_torch(ins[0])
        res = O.to_torch(ins[1]) if len(ins) > 1 else None
        if not (_PANEL and self.use_hip and x.is_cuda and x.dim() == 4 and x.shape[3] == self.cin):
            return None
        if not panel_eligible(self.kh, self.kw, self.sh, self.sw, self.pads_for(x.shape[1], x.shape[2]), self.cin,
                              self.cout, self.act, self.post, self.c4):
            return None
        if res is not None and tuple(res.shape) != tuple(x.shape[:3]) + (self.cout,):
            return None                 # (a broadcast residual: the tile path expands it)
        from ..ops import hip, tuned_choice
        forms = hip().conv1x1_panel_forms(x.shape[0] * x.shape[1] * x.shape[2], self.cout, self.cin)
        if not forms:
            return None
        # option 0 is today's launch, and the pick during capture or without autotuning
        opts = {i: (lambda i=i: self(ctx, node, ins, panel_pick=i)) for i in range(len(forms) + 1)}
        pick = tuned_choice(panel_key(x.shape, self.cout, res is not None, self.act), opts, default=0)
        return pick if pick in opts else 0

    def __call__(self, ctx, node, ins, panel_pick=None):
        x = O.to_torch(ins[0])
        res = O.to_torch(ins[1]) if len(ins) > 1 else None
        pt, pb, pl, pr = self.pads_for(x.shape[1], x.shape[2])
        if not self.use_hip or x.shape[3] != self.cin:
            return self._torch(x, res, (pt, pb, pl, pr))
        if panel_pick is None:
            panel_pick = self.panel_choice(ctx, node, ins)
        from ..ops import ACT, hip, tuned_config
        if self.c4:
            # fp32 RGB request -> zero-bordered bf16 RGBA sized for the padded
            # (khp x 8) filter; the conv itself then has no padding
            ho, wo = self.out_hw(x.shape[1], x.shape[2], (pt, pb, pl, pr))
            hp, wp = (ho - 1) * self.sh + self.khp, (wo - 1) * self.sw + 8
            x = hip().ingest_c4_padded(x.float().contiguous(), hp, wp, pt, pl)
            pt = pb = pl = pr = 0
        elif self.cin % 8 != 0:
            x = x.float().contiguous()            # generic: fp32 operand gather + cast in-kernel
        else:
            x = _to_bf16(x).contiguous()
        H = hip()
        n, h, w, _ = x.shape
        kh, kw = (self.khp, 8) if self.c4 else (self.kh, self.kw)
        ho, wo = self.out_hw(h, w, (pt, pb, pl, pr), kh, kw)
        if res is not None:
            # the kernel reads one residual element per output element: a broadcast operand
            # ([B,1,1,C], [1,1,1,C], a scalar) is expanded first
            res = _residual_for(res, (n, ho, wo, self.cout))
            if res is None:
                return _add_residual_unfused(self, ctx, node, ins[0], O.to_torch(ins[1]))
            res = _to_bf16(res).contiguous()
        M = n * ho * wo
        args = (x, self.w, self.b, res, kh, kw, self.sh, self.sw, pt, pb, pl, pr, ACT[self.act])
        out = torch.empty((n, ho, wo, self.cout), device=x.device, dtype=BF16)
        K = kh * 32 if self.c4 else kh * kw * self.cin
        dma = not self.c4 and self.cin % 8 == 0      # bf16 dense/im2col operands -> DMA-ring configs apply
        # pipelined cgemm kernel applies (im2col / dense with C % 64, or the padded RGBA stem)
        aligned = (dma and self.cin % 64 == 0) or self.c4
        # the halo kernel's tile origin reaches at most 2 rows / columns into the top / left padding
        # (halo.hip halo_supported)
        halo_shape = aligned and not self.c4 and kh == 3 and kw == 3 and self.sh == 1
        halo = halo_shape and self.sw == 1 and pt <= 2 and pl <= 2
        # a pick is only valid for the launches that share its candidate list: a column stride that
        # differs from the row stride, or padding that rules the halo configs out, is part of the key
        # (appended only then, so the keys of square-stride convs -- the committed table's -- are unchanged)
        key = ("conv", tuple(x.shape), x.dtype, self.cout, kh, kw, self.sh, res is not None, self.act,
               self.post_mode) + ((self.sw,) if self.sw != self.sh else ()) + \
            (("nohalo",) if halo_shape and self.sw == 1 and not halo else ())
        kw_post, outs = _post_kwargs(self, out)
        run = lambda c, s: H.conv2d(*args, cfg=c, out=out, splits=s, **kw_post)  # noqa
        # (ReLU6 and hard-swish are igemm epilogues only: those launches tune over the igemm configs)
        flags = {"relu6": True} if self.act in IGEMM_ONLY_ACTS else {}
        if panel_pick:
            # a wide expand conv on the row-panel kernel (kernels/panel.hip): form panel_pick of its forms
            bm, ns = H.conv1x1_panel_forms(M, self.cout, self.cin)[panel_pick - 1]
            H.conv1x1_panel(x, self.w, self.b, res, ACT[self.act], bm, ns, out=out)
            return outs
        cfg, splits = tuned_config(key, M, self.cout, run, K, dma, aligned, halo=halo,
                                   cgemm_only=self.post is not None, stem=self.c4, **flags)
        run(cfg, splits)
        return outs


class FusedDepthwiseConv(_Window):
    """DepthwiseConv2dNative (channel multiplier 1)(+folded BN/bias)(+act).
    The filter stays fp32 on both paths: [KH][KW][C], which the kernel reads as
    [KH*KW][C] (9 C floats for a 3x3: rounding it to bf16 would cost 2^-9
    relative error for no saving)."""

    MAX_K = 7                       # kernels/dwconv.hip kMaxTaps

    def __init__(self, w_hwc: torch.Tensor, bias: torch.Tensor, strides, padding: str, pads, act: str,
                 device: torch.device, use_hip: bool, name: str):
        kh, kw, self.c = w_hwc.shape
        self._set_window(kh, kw, strides, padding, pads)
        self.act = act
        self.use_hip = use_hip
        self.name = name
        self.device = device
        self.w = to_device(w_hwc.float().contiguous(), device)
        self.b = to_device(bias.float(), device)

    @classmethod
    def hip_ok(cls, kh: int, kw: int, c: int) -> bool:
        return c % 8 == 0 and kh <= cls.MAX_K and kw <= cls.MAX_K

    def _torch(self, x, pads):
        """The fp32 reference conv (no activation): the filter as [kh, kw, 1, C], C groups."""
        w = self.w.to(x.device).reshape(self.kh, self.kw, 1, self.c)
        return _grouped_conv_torch(x.float(), w, self.b.to(x.device), (self.sh, self.sw), pads, self.c)

    def __call__(self, ctx, node, ins):
        x = O.to_torch(ins[0])
        pt, pb, pl, pr = self.pads_for(x.shape[1], x.shape[2])
        n, h, w, _ = x.shape
        ho, wo = self.out_hw(h, w, (pt, pb, pl, pr))
        if not self.use_hip:
            return [_ref_act(self._torch(x, (pt, pb, pl, pr)), self.act).contiguous()]
        from ..ops import ACT, hip, tuned_choice
        H = hip()
        x = _to_bf16(x).contiguous()
        out = torch.empty((n, ho, wo, self.c), device=x.device, dtype=BF16)

        def run(strip):
            return H.dwconv2d(x, self.w, self.b, self.kh, self.kw, self.sh, self.sw, pt, pl, ho, wo, ACT[self.act],
                              out, strip)
        auto = H.dwconv_strip(n, ho, wo, self.c, self.kh, self.kw, self.sh, self.sw)
        if auto == 0:
            forms = H.dwconv_forms(n, ho, wo, self.c, self.kh, self.kw, self.sh, self.sw)
            if len(forms) == 1:
                return [run(0)]     # the generic kernel has one form
            # 5x5: the generic kernel or a strip kernel (2 or 4 rows per thread; bit-equal results), timed
            # per shape; its own key, so a 3x3 entry of the cached table can never answer for it
            key = ("dwconv5x5", tuple(x.shape), self.sh, self.sw, pt, pl, ho, wo, self.act)
            pick = tuned_choice(key, {int(f): (lambda f=int(f): run(f)) for f in forms}, default=0)
            return [run(pick)]
        # output rows per thread (kernels/launch.h kDwStripShort / kDwStripTall), timed per shape
        key = ("dwconv", tuple(x.shape), self.kh, self.kw, self.sh, self.sw, pt, pl, ho, wo, self.act)
        pick = tuned_choice(key, {2: lambda: run(2), 8: lambda: run(8)}, default=auto)
        return [run(pick)]


class FusedDepthwiseLN:
    """``_LayerNorm(_FusedDepthwiseConv2D(x))`` for a 7x7 / stride-1 depthwise
    conv without activation: the opening of a ConvNeXt block as one launch
    (kernels/dwln.hip), the conv result in fp32 up to the one rounding of the
    normalised output.  It owns the two ops it replaces (``dw``, ``ln``: their
    weights are its weights) and runs them as they were for an input that is
    not NHWC with C channels, for a shape the kernel does not take, and under
    ``TFSERVE_DWLN=0`` (A/B only)."""

    children = ("dw", "ln")             # placement.weight_refs

    def __init__(self, dw: "FusedDepthwiseConv", ln, use_hip: bool, name: str):
        self.dw, self.ln = dw, ln
        self.c = dw.c
        self.eps = ln.eps
        self.use_hip = use_hip
        self.name = name

    @staticmethod
    def shape_ok(dw: "FusedDepthwiseConv") -> bool:
        """What kernels/dwln.hip takes, the channel count aside."""
        return dw.kh == 7 and dw.kw == 7 and dw.sh == 1 and dw.sw == 1 and dw.act == "none"

    def _pair(self, ctx, node, x):
        return self.ln(ctx, node, self.dw(ctx, node, [x]))

    def __call__(self, ctx, node, ins):
        x = O.to_torch(ins[0])
        if x.dim() != 4 or x.shape[3] != self.c:
            return self._pair(ctx, node, x)
        dw = self.dw
        pt, pb, pl, pr = dw.pads_for(x.shape[1], x.shape[2])
        n, h, w, _ = x.shape
        ho, wo = dw.out_hw(h, w, (pt, pb, pl, pr))
        gamma, beta = self.ln.params(self.c)
        if not self.use_hip:
            y = dw._torch(x, (pt, pb, pl, pr))
            return [F.layer_norm(y, (self.c,), gamma.to(x.device), beta.to(x.device), self.eps).contiguous()]
        from ..ops import hip
        H = hip()
        if (os.environ.get("TFSERVE_DWLN", "1") == "0" or not x.is_cuda or ho < 1 or wo < 1 or
                not H.dwconv_ln_supported(n, ho, wo, self.c, 7, 7, 1, 1)):
            return self._pair(ctx, node, x)
        x = _to_bf16(x).contiguous()
        out = torch.empty((n, ho, wo, self.c), device=x.device, dtype=BF16)
        return [H.dwconv_ln(x, dw.w, dw.b, gamma, beta, self.eps, pt, pl, ho, wo, out)]


GCONV_CG = (4, 8, 16, 32)         # kernels/gconv.hip: channels per group, in == out


def gconv_ksteps(cg: int) -> int:
    """32-deep MFMA k-steps per output (kernels/launch.h gconv_ksteps)."""
    return (9 * cg + 31) // 32


def pack_grouped_filter(w_hwio: torch.Tensor, cg: int) -> torch.Tensor:
    """The [3][3][cg][C] filter of a grouped conv with cg outputs per group, as
    bf16 in the MFMA fragment order of kernels/gconv.hip (launch.h):
    [C / cg groups][k-steps][column tiles][64 lanes][8], element j of lane l =
    B[k = 32 ks + 8 (l >> 4) + j][col = 16 nt + (l & 15)] with k = tap * cg +
    channel; zeros where k >= 9 cg (the K padding) and where col >= cg."""
    kh, kw, ci, c = w_hwio.shape
    assert (kh, kw, ci) == (3, 3, cg) and c % cg == 0 and cg in GCONV_CG
    g, ks, nt = c // cg, gconv_ksteps(cg), 2 if cg == 32 else 1
    b = torch.zeros(g, ks * 32, nt * 16, dtype=torch.float32, device=w_hwio.device)
    b[:, :9 * cg, :cg] = w_hwio.float().reshape(9 * cg, g, cg).permute(1, 0, 2)
    # [g][ks][q][j][nt][m] -> [g][ks][nt][q][m][j], lane = 16 q + m
    b = b.reshape(g, ks, 4, 8, nt, 16).permute(0, 1, 4, 2, 5, 3)
    return b.contiguous().to(BF16).reshape(-1)


class FusedGroupedConv(_Window):
    """Grouped Conv2D (a filter whose in-depth is C / groups)(+folded BN/bias)(+act
    none | relu).  The fp32 HWIO filter serves the CPU reference and the torch
    paths; the kernel (kernels/gconv.hip: 3x3, equal strides 1 | 2, cg inputs
    and outputs per group, cg in 4 | 8 | 16 | 32) reads it packed as bf16 MFMA
    fragments.  Any other shape runs torch's grouped conv on the device."""

    def __init__(self, w_hwio: torch.Tensor, bias: torch.Tensor, strides, padding: str, pads, act: str,
                 device: torch.device, use_hip: bool, name: str, channels: int):
        kh, kw, self.cg, self.cout = w_hwio.shape
        self._set_window(kh, kw, strides, padding, pads)
        self.c = channels                           # input channels the pass saw: groups * cg
        self.groups = channels // self.cg
        self.cgo = self.cout // self.groups
        self.act = act
        self.use_hip = use_hip
        self.name = name
        self.device = device
        self.kernel = use_hip and self.hip_ok(self.kh, self.kw, self.cg, self.cgo, channels, strides)
        self.b = to_device(bias.float(), device)
        if self.kernel:
            self.w = to_device(pack_grouped_filter(w_hwio, self.cg), device)
        else:
            self.w_ref = to_device(w_hwio.float().contiguous(), device)

    @staticmethod
    def hip_ok(kh: int, kw: int, cg_in: int, cg_out: int, c: int, strides) -> bool:
        """What kernels/gconv.hip takes (launch.h gconv_supported)."""
        return (kh == 3 and kw == 3 and cg_in == cg_out and cg_in in GCONV_CG and c % 8 == 0 and c % cg_in == 0 and
                strides[0] == strides[1] and strides[0] in (1, 2))

    def _hwio(self) -> torch.Tensor:
        if hasattr(self, "w_ref"):
            return self.w_ref
        # back from the fragments (bf16 values): [g][ks][nt][q][m][j] -> [g][k][col]
        g, ks, nt = self.groups, gconv_ksteps(self.cg), 2 if self.cg == 32 else 1
        b = self.w.float().reshape(g, ks, nt, 4, 16, 8).permute(0, 1, 3, 5, 2, 4).reshape(g, ks * 32, nt * 16)
        return b[:, :9 * self.cg, :self.cg].permute(1, 0, 2).reshape(3, 3, self.cg, self.cout)

    def _torch(self, x, pads):
        """Conv2D's own semantics for this input (ops._conv2d: groups from the
        input's channel count), fp32 accumulation; bf16 out on the device."""
        xf = x.float()
        y = _grouped_conv_torch(xf, self._hwio().to(x.device), self.b.to(x.device), (self.sh, self.sw), pads,
                                x.shape[3] // self.cg)
        y = _ref_act(y, self.act).contiguous()
        return [y.to(BF16) if self.use_hip else y]

    def __call__(self, ctx, node, ins):
        x = O.to_torch(ins[0])
        pads = self.pads_for(x.shape[1], x.shape[2])
        if not self.kernel or x.shape[3] != self.c or os.environ.get("TFSERVE_GCONV", "1") == "0":
            return self._torch(x, pads)
        from ..ops import ACT, hip
        pt, _pb, pl, _pr = pads
        n, h, w, _ = x.shape
        ho, wo = self.out_hw(h, w, pads)
        x = _to_bf16(x).contiguous()
        out = torch.empty((n, ho, wo, self.cout), device=x.device, dtype=BF16)
        return [hip().gconv2d(x, self.w, self.b, self.cg, self.sh, pt, pl, ho, wo, ACT[self.act], out)]


class FusedDualConv:
    """``act(conv1x1(h) + conv1x1_stride(x) + b)`` as ONE GEMM over the
    K-concatenated operands [h | x(strided)] and weights [W_h ; W_x] (cgemm
    dual-source A mode): a ResNet bottleneck's expand conv and its projection
    shortcut, without writing / re-reading the projection's output."""

    def __init__(self, conv_h: FusedConv, conv_x: FusedConv, act: str, device, use_hip: bool, name: str):
        self.c1, self.c2 = conv_h.cin, conv_x.cin
        self.cout = conv_h.cout
        self.sh, self.sw = conv_x.sh, conv_x.sw
        self.act = act
        self.use_hip = use_hip
        self.name = name
        self.device = device
        if use_hip:
            # [Cout][C1 + C2] bf16, concatenated on the device (no host round trip)
            w = torch.cat([conv_h.w[:, :self.c1], conv_x.w[:, :self.c2]], dim=1)
            self.w = to_device(_pad_k(w, 8), device)
            self.b = (conv_h.b + conv_x.b).contiguous()
        else:
            self.w1, self.w2 = conv_h.w_ref, conv_x.w_ref
            self.b_ref = conv_h.b_ref + conv_x.b_ref

    post = None
    post_mode = None
    set_post = FusedConv.set_post

    def post_ok(self) -> bool:
        return self.cout % 8 == 0

    def __call__(self, ctx, node, ins):
        h, x = O.to_torch(ins[0]), O.to_torch(ins[1])
        if not self.use_hip:
            y = h.float() @ self.w1.reshape(self.c1, self.cout)
            xs = x.float()[:, ::self.sh, ::self.sw, :]
            y = y + xs @ self.w2.reshape(self.c2, self.cout) + self.b_ref
            return _with_post(self, _ref_act(y, self.act).contiguous())
        from ..ops import ACT, hip, tuned_config
        H = hip()
        xs = x[:, ::self.sh, ::self.sw, :]
        if h.dim() != 4 or tuple(xs.shape[:3]) != tuple(h.shape[:3]):
            # the two convs' outputs only broadcast against each other (a [B,1,1,C] projection): the
            # kernel reads both sources at every output pixel, so the sum is taken with torch
            w = self.w.float()
            y = h.float() @ w[:, :self.c1].t() + xs.float() @ w[:, self.c1:self.c1 + self.c2].t() + self.b
            return [o.to(BF16) for o in _with_post(self, _ref_act(y, self.act).contiguous())]
        h, x = _to_bf16(h).contiguous(), _to_bf16(x).contiguous()
        n, ho, wo, _ = h.shape
        out = torch.empty((n, ho, wo, self.cout), device=h.device, dtype=BF16)
        key = ("dual", tuple(h.shape), tuple(x.shape), self.cout, self.sh, self.act, self.post_mode) + \
            ((self.sw,) if self.sw != self.sh else ())
        kw_post, outs = _post_kwargs(self, out)
        run = lambda c, s: H.conv2d_dual(h, x, self.w, self.b, self.sh, self.sw, ACT[self.act], c, out, s,  # noqa
                                         **kw_post)
        cfg, splits = tuned_config(key, n * ho * wo, self.cout, run, self.c1 + self.c2, True, True, cgemm_only=True)
        run(cfg, splits)
        return outs


class FusedMatMul:
    """``pad_n``: the consumers accept a row-strided [M, N] view, so an N that
    is not a multiple of 8 (ResNet's 1001 classes) is computed as ceil8(N)
    columns (zero weight rows) into an [M, ceil8(N)] buffer and returned as
    its first N columns: the pipelined cgemm kernel applies (it needs N % 8 ==
    0) instead of igemm + split-K reduce."""

    def __init__(self, w_kn: torch.Tensor, bias: Optional[torch.Tensor], act: str, out_f32: bool,
                 device, use_hip: bool, name: str, pad_n: bool = False):
        self.k, self.n = w_kn.shape
        self.act = act
        self.out_f32 = out_f32
        self.use_hip = use_hip and self.k % 8 == 0
        self.name = name
        b = bias if bias is not None else zeros(self.n, w_kn)
        self.np = -(-self.n // 8) * 8 if (pad_n and self.n % 8 and self.k % 64 == 0) else self.n
        self.device = device
        # the fp32 weights as given, kept until the compile passes are over
        # (defer_layernorm folds a LayerNorm's gamma / beta into them; then
        # release_weight_sources drops them)
        self._w_src = w_kn if self.use_hip else None
        if self.use_hip:
            w_nk = w_kn.t().contiguous()
            if self.np != self.n:
                w_nk = torch.cat([w_nk, torch.zeros(self.np - self.n, self.k, dtype=w_nk.dtype, device=w_nk.device)])
                b = torch.cat([b.float().reshape(-1), zeros(self.np - self.n, b)])
            self.w = to_device(_pad_k(w_nk, 8).to(BF16), device)
            self.b = to_device(b.float(), device)
        else:
            self.w_ref = to_device(w_kn.float(), device)
            self.b_ref = to_device(b.float(), device)

    def __call__(self, ctx, node, ins):
        x = O.to_torch(ins[0])
        res = O.to_torch(ins[1]) if len(ins) > 1 else None
        if not self.use_hip:
            y = x.float() @ self.w_ref.to(x.device) + self.b_ref.to(x.device)
            if res is not None:
                y = y + res.float()
            y = _ref_act(y, self.act)
            return [y if self.out_f32 or not x.is_cuda else y.to(BF16)]
        from ..ops import ACT, hip, tuned_config
        H = hip()
        x = _to_bf16(x)
        if res is not None:
            # one residual element per output element: a [1, N] or [N] operand is expanded first
            res = _residual_for(res, list(x.shape[:-1]) + [self.n])
            if res is None:
                return _add_residual_unfused(self, ctx, node, ins[0], O.to_torch(ins[1]))
        if not (x.dim() == 2 and x.stride(1) == 1 and x.stride(0) % 8 == 0 and res is None):
            # (a row-strided 2-D view -- BERT's pooler reading each sequence's
            # first token out of [B, S, H] -- is read in place: no copy kernel)
            x = x.contiguous()
        if res is not None:
            res = _to_bf16(res).contiguous()
        M = x.shape[0] if x.dim() == 2 else x.numel() // self.k
        padded = self.np != self.n and res is None and x.dim() == 2
        n = self.np if padded else self.n
        w, b = (self.w, self.b) if padded or self.np == self.n else (self.w[:self.n], self.b[:self.n])
        shape = list(x.shape[:-1]) + [n]
        out = torch.empty(shape, device=x.device, dtype=torch.float32 if self.out_f32 else BF16)
        key = ("mm", M, n, self.k, res is not None, self.out_f32, self.act) + \
            ((x.stride(0),) if not x.is_contiguous() else ())
        run = lambda c, s: H.linear(x, w, b, res, ACT[self.act], c, self.out_f32, 1.0, out, s)  # noqa
        cfg, splits = tuned_config(key, M, n, run, self.k, True, self.k % 64 == 0)
        y = run(cfg, splits)
        return [y[:, :self.n] if padded else y]


class DeferredLNMatMul(FusedMatMul):
    """A _FusedMatMul / _FusedQKV around LayerNorms that are never stored
    (``defer_layernorm``): ``LN(z) = (z - mean) * rstd * gamma + beta`` of a
    GEMM output ``z`` is applied inside the GEMMs that read it, from row
    statistics the producing GEMM's epilogue emits ([M][P][2] fp32 (sum, sum of
    squares) partials, one per row and producer column block).

    * ``emit``: this GEMM's bf16 output rows feed a deferred LayerNorm: it also
      returns their partials (output 1).
    * ``a_ln`` = (eps,): input 0 is a pre-LayerNorm ``z`` (statistics at input
      ``a_pos``).  ``LN(z) @ W + b = rstd * (z @ W' - mean * colsum(W')) + b'``
      with ``W' = diag(gamma) W`` (folded in fp32, then rounded once to bf16),
      ``b' = b + beta @ W`` and ``colsum`` = the per-column sums of the bf16
      ``W'`` -- the GEMM runs on ``z`` unchanged.
    * ``r_ln`` = (gamma, beta, eps): the residual (input 1) is a pre-LayerNorm
      ``z`` (statistics at input ``r_pos``), normalised per element in the
      epilogue.

    One kernel per GEMM (kernels/cgemm_impl.h epilogue_lnx, bindings
    ``linear_lnx``): the 23 of 24 encoder LayerNorm launches of BERT-base
    whose inputs and outputs are GEMMs disappear (the last one feeds the
    pooler's strided view and stays).  Round 3's fold spilled registers in
    the 8-wave tiles (profiles/round3/ln_fold.md); this one does not (LDS
    column vectors, statistics fetched before the K loop, a separate LNX
    kernel build), and still only breaks even -- see defer_layernorm."""

    emit = False
    has_res = False
    a_ln = None
    a_pos = None
    r_ln = None
    r_pos = None
    colsum = None

    @classmethod
    def of(cls, node) -> "DeferredLNMatMul":
        """The node's impl as a DeferredLNMatMul (converted in place the first
        time, while its inputs are still [x] or [x, residual])."""
        mm = node.attr("_impl")
        if isinstance(mm, DeferredLNMatMul):
            return mm
        d = cls.__new__(cls)
        d.__dict__.update(mm.__dict__)
        d.has_res = len(node.inputs) > 1
        node.attrs["_impl"] = d
        return d

    def fold_input_ln(self, gamma: torch.Tensor, beta: torch.Tensor, eps: float):
        w_kn = self._w_src.float()
        g = gamma.detach().float().reshape(-1).to(w_kn.device)
        bt = beta.detach().float().reshape(-1).to(w_kn.device)
        b = self.b.detach().float().to(w_kn.device)
        wf = w_kn * g[:, None]
        self.w = to_device(_pad_k(wf.t().contiguous(), 8).to(BF16), self.device)
        self.b = to_device((b + bt @ w_kn).float(), self.device)
        self.colsum = self.w.float().sum(1).contiguous()
        self.a_ln = (float(eps),)

    def _stats(self, st: torch.Tensor, length: int, eps: float):
        s = st.float().sum(1)
        mean = s[:, 0] / length
        var = (s[:, 1] / length - mean * mean).clamp_min(0)
        return mean, torch.rsqrt(var + eps)

    def __call__(self, ctx, node, ins):
        x = _to_bf16(O.to_torch(ins[0])).contiguous()
        res = _to_bf16(O.to_torch(ins[1])).contiguous() if self.has_res else None
        a_st = O.to_torch(ins[self.a_pos]) if self.a_ln is not None else None
        r_st = O.to_torch(ins[self.r_pos]) if self.r_ln is not None else None
        M = x.numel() // self.k
        shape = list(x.shape[:-1]) + [self.n]
        if not x.is_cuda:
            return self._reference(x, res, a_st, r_st, M, shape)
        from ..ops import ACT, hip, tuned_config
        H = hip()
        out = torch.empty(shape, device=x.device, dtype=torch.float32 if self.out_f32 else BF16)
        ra = self.r_ln
        key = ("mmx", M, self.n, self.k, res is not None, self.out_f32, self.act, self.a_ln is not None,
               ra is not None, self.emit)

        def run(c, _s):
            return H.linear_lnx(x, self.w, self.b, res, ACT[self.act], c, self.out_f32, out,
                                a_st, self.colsum, self.a_ln[0] if self.a_ln else 1e-12,
                                r_st, ra[0] if ra else None, ra[1] if ra else None, ra[2] if ra else 1e-12,
                                self.emit)
        # linear_lnx takes cgemm configs only: the untimed pick (autotuning off, or under graph
        # capture) must be one of them, not the igemm heuristic
        cfg, _ = tuned_config(key, M, self.n, run, self.k, True, True, cgemm_only=True, no_split=True, ln=True)
        y, st = run(cfg, 1)
        return [y, st] if self.emit else [y]

    def _reference(self, x, res, a_st, r_st, M, shape):
        """The kernel's math in fp32 torch (CPU tensors; tests)."""
        acc = x.float().reshape(M, self.k) @ self.w.float().cpu()[:, :self.k].t()
        if self.a_ln is not None:
            mean, rstd = self._stats(a_st.cpu(), self.k, self.a_ln[0])
            acc = rstd[:, None] * (acc - mean[:, None] * self.colsum.cpu()[None, :])
        y = acc + self.b.float().cpu()
        if res is not None:
            r = res.float().reshape(M, self.n)
            if self.r_ln is not None:
                g, b, eps = self.r_ln
                mean, rstd = self._stats(r_st.cpu(), self.n, eps)
                r = (r - mean[:, None]) * rstd[:, None] * g.cpu() + b.cpu()
            y = y + r
        y = _ref_act(y, self.act)
        yb = y.to(BF16) if not self.out_f32 else y
        outs = [yb.reshape(shape)]
        if self.emit:
            f = yb.float()
            outs.append(torch.stack([f.sum(1), (f * f).sum(1)], 1).reshape(M, 1, 2))
        return outs


def _lnx_gemm_ok(impl, k: int) -> bool:
    return isinstance(impl, FusedMatMul) and impl.use_hip and impl.np == impl.n and impl.k == k and \
        impl.k % 64 == 0 and impl.n % 32 == 0 and getattr(impl, "_w_src", None) is not None


def defer_layernorm(g, order, fed, fetch_refs, device, opts):
    """_LayerNorm(z) with z = a _FusedMatMul output read by nothing else, and
    every reader of the LayerNorm a _FusedMatMul / _FusedQKV taking it as
    input 0 (A) or input 1 (residual): the LayerNorm node goes away -- the
    producer emits z's row statistics, the readers take z plus the
    statistics (DeferredLNMatMul).  Opt-in (TFSERVE_DEFER_LN=1): on
    MI355X it measured level with the LayerNorm kernels at b32 (engine
    1.560 / 1.568 vs 1.544 ms), behind at b1 (0.624 vs 0.585 ms) and in the
    BERT serving bench (25.9k vs 27.1k RPC/s, profiles/round5/s15): the
    epilogue work it adds to the four GEMMs (1.5-2.5 us each in isolation,
    scripts/lnx_probe.py) costs about what the LayerNorm launches did."""
    c = _Ctx(g, order, fed, fetch_refs, device, opts)
    if not c.use_hip or os.environ.get("TFSERVE_DEFER_LN", "0") != "1":
        return
    for name in order:
        ln_node = g.nodes.get(name)
        if ln_node is None or ln_node.op != "_LayerNorm" or ln_node.name in c.fetch_nodes:
            continue
        ln = ln_node.attr("_impl")
        if ln is None or not getattr(ln, "use_hip", False):
            continue
        C = ln.g.numel()
        src, sidx = ln_node.inputs[0]
        prod = g.nodes.get(src)
        if prod is None or sidx != 0 or prod.op not in ("_FusedMatMul", "_FusedQKV"):
            continue
        pm = prod.attr("_impl")
        if not isinstance(pm, FusedMatMul) or not pm.use_hip or pm.n != C or pm.np != C or pm.out_f32 or \
                pm.k % 64 or C % 32 or c.only_consumer(prod.name) is not ln_node:
            continue
        readers = c.cons.get(ln_node.name, [])
        ok = bool(readers)
        for cname, pos, oidx in readers:
            cn = g.nodes[cname]
            ci = cn.attr("_impl")
            if oidx != 0 or cn.op not in ("_FusedMatMul", "_FusedQKV") or ci is None:
                ok = False
            elif pos == 0:
                ok = ok and _lnx_gemm_ok(ci, C) and getattr(ci, "a_ln", None) is None and \
                    not (len(cn.inputs) > 1 and cn.inputs[1] == (ln_node.name, 0))
            elif pos == 1:
                ok = ok and isinstance(ci, FusedMatMul) and ci.use_hip and ci.n == C and ci.np == C and \
                    ci.k % 64 == 0 and ci.n % 32 == 0 and getattr(ci, "r_ln", None) is None
            else:
                ok = False
        if not ok:
            continue
        DeferredLNMatMul.of(prod).emit = True
        z = (prod.name, 0)
        stats = (prod.name, 1)
        for cname, pos, _o in readers:
            cn = g.nodes[cname]
            d = DeferredLNMatMul.of(cn)
            cn.inputs[pos] = z
            if pos == 0:
                d.fold_input_ln(ln.g, ln.b, ln.eps)
                d.a_pos = len(cn.inputs)
            else:
                d.r_ln = (ln.g, ln.b, float(ln.eps))
                d.r_pos = len(cn.inputs)
            cn.inputs.append(stats)
        del g.nodes[ln_node.name]
        c.refresh()


def ln_weight_frags(w_nk: torch.Tensor) -> torch.Tensor:
    """[N][K] -> the fragment-major layout kernels/lngemm.hip streams: for
    16-row n-tile nt and 32-deep K-step t, one contiguous KB whose lane l =
    16 q + r holds w[16 nt + r][32 t + 8 q .. + 8] (a v_mfma_f32_16x16x32_bf16
    B fragment).  Returned as a contiguous [N][K] tensor."""
    n, k = w_nk.shape
    return w_nk.reshape(n // 16, 16, k // 32, 4, 8).permute(0, 2, 3, 1, 4).contiguous().reshape(n, k)


class MatMulLN:
    """A _FusedMatMul with a residual input whose only reader is a _LayerNorm
    over its N columns (BERT's attention-output projection + residual +
    LayerNorm): one ``hip().linear_ln`` launch (kernels/lngemm.hip: a
    workgroup owns whole rows, so the row statistics stay on the CU and the
    GEMM output is never re-read), or the two launches -- timed per shape
    (ops.tuned_choice: option 0 = split, 1 / 2 / 3 = the fused kernel with
    32 / 64 / 16 rows per workgroup).  The weights stay in the children
    (parallel/weights.py binds them there).  Request path: BERT Predict
    (/root/reference/protos/tensorflow_serving/apis/predict.proto:12-40)."""

    children = ("mm", "ln")
    BM = {1: 32, 2: 64, 3: 16}

    def __init__(self, mm: "FusedMatMul", ln):
        self.mm, self.ln = mm, ln
        self.use_hip = mm.use_hip and ln.use_hip
        self.name = mm.name
        # the kernel's fragment-major copy of the weights (a weight of this op:
        # built from mm.w on its device, meta on a follower until bound)
        self.w_frag = ln_weight_frags(mm.w[:, :mm.k])

    @staticmethod
    def fusable(mm, ln) -> bool:
        from ..ops import hip
        return isinstance(mm, FusedMatMul) and mm.use_hip and getattr(ln, "use_hip", False) and \
            mm.act == "none" and not mm.out_f32 and mm.np == mm.n and mm.n == ln.g.numel() and \
            mm.n in (512, 768, 1024) and mm.k % 128 == 0 and hip().linear_ln_supported(1, mm.n, mm.k, 32)

    def __call__(self, ctx, node, ins):
        mm, ln = self.mm, self.ln

        def split():
            return ln(ctx, node, mm(ctx, node, ins))
        x = O.to_torch(ins[0])
        res = O.to_torch(ins[1]) if len(ins) > 1 else None
        if not (self.use_hip and x.is_cuda and x.shape[-1] == mm.k and
                (res is None or tuple(res.shape) == tuple(x.shape[:-1]) + (mm.n,))):
            return split()
        from ..ops import hip, tuned_choice
        H = hip()
        xb = _to_bf16(x).contiguous()
        rb = None if res is None else _to_bf16(res).contiguous()
        M = xb.numel() // mm.k
        opts = {0: split}
        for o, bm in self.BM.items():
            if H.linear_ln_supported(M, mm.n, mm.k, bm):
                opts[o] = (lambda bm=bm: [H.linear_ln(xb, self.w_frag, mm.b, rb, ln.g, ln.b, ln.eps, bm)])
        key = ("mmln", M, mm.n, mm.k, rb is not None)
        pick = tuned_choice(key, opts, default=0)
        return opts.get(pick, split)()


def fuse_matmul_layernorm(g, order, fed, fetch_refs, device, opts):
    """_LayerNorm(_FusedMatMul(x, residual)) with the LayerNorm the GEMM
    output's only reader -> _FusedMatMulLN (MatMulLN).  GPU only, opt-in
    (TFSERVE_MATMUL_LN=1): measured slower than the two launches on MI355X.
    BERT-base b32 attention output (4096 x 768 x 768, graph-captured, L2-cold
    operands): fused 21.1 us (16 rows per workgroup) / 23.2 us (32) against
    11.9 + 5.8 = 17.7 us; FFN2 (K = 3072) 63.2 against 37.5 us
    (profiles/round6/r6j/probe.log).  A workgroup that owns whole rows must
    stream the whole weight matrix (1.2 MB) through one CU, and one CU takes in
    ~60 GB/s even with fragment-major weights (42-46 us per workgroup with
    [N][K] fragment loads, profiles/round6/r6h).  The opt-in defer_layernorm
    (TFSERVE_DEFER_LN=1) takes precedence."""
    c = _Ctx(g, order, fed, fetch_refs, device, opts)
    if not c.use_hip or os.environ.get("TFSERVE_MATMUL_LN", "0") != "1" or \
            os.environ.get("TFSERVE_DEFER_LN", "0") == "1":
        return
    for name in order:
        ln_node = g.nodes.get(name)
        if ln_node is None or ln_node.op != "_LayerNorm" or len(ln_node.inputs) != 1:
            continue
        src, sidx = ln_node.inputs[0]
        prod = g.nodes.get(src)
        if prod is None or sidx != 0 or prod.op != "_FusedMatMul" or c.only_consumer(prod.name) is not ln_node:
            continue
        mm, ln = prod.attr("_impl"), ln_node.attr("_impl")
        if ln is None or not MatMulLN.fusable(mm, ln):
            continue
        ln_node.op = "_FusedMatMulLN"
        ln_node.attrs = {"_impl": MatMulLN(mm, ln)}
        ln_node.inputs = list(prod.inputs)
        ln_node.ctrl = _merge_ctrl([prod, ln_node])
        del g.nodes[prod.name]
        c.refresh()


def release_weight_sources(g, order, fed, fetch_refs, device, opts):
    """Drops the fp32 weight copies the GEMM ops kept for defer_layernorm."""
    for n in g.nodes.values():
        impl = n.attrs.get("_impl") if n.attrs else None
        if isinstance(impl, FusedMatMul):
            impl._w_src = None


class DenseSoftmax:
    """softmax(x @ W + b) over a few classes (BERT's classifier: 2 labels):
    one kernel (misc.hip dense_softmax_kernel) from the fp32 pooled rows,
    instead of cast + a GEMM launch with mostly empty tiles + torch softmax."""
    children = ("mm",)          # placement.weight_refs: the classifier weights live in mm

    def __init__(self, mm: "FusedMatMul"):
        self.mm = mm

    def __call__(self, ctx, node, ins):
        x = O.to_torch(ins[0])
        mm = self.mm
        if mm.use_hip and x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.is_contiguous() and \
                mm.k % 4 == 0:
            from ..ops import hip
            return [hip().dense_softmax(x, mm.w, mm.b, mm.n)]
        y = mm(ctx, node, [x])[0]
        return [torch.softmax(y.float(), dim=-1)]


def fuse_dense_softmax(g, order, fed, fetch_refs, device, opts):
    """Softmax(_FusedMatMul(x)) with <= 16 classes, no activation / residual and
    the logits used by nothing else -> _DenseSoftmax(x)."""
    c = _Ctx(g, order, fed, fetch_refs, device, opts)
    for name in order:
        sm = g.nodes.get(name)
        if sm is None or sm.op != "Softmax" or len(sm.inputs) != 1:
            continue
        mm = g.nodes.get(sm.inputs[0][0])
        if mm is None or mm.op != "_FusedMatMul" or sm.inputs[0][1] != 0 or len(mm.inputs) != 1:
            continue
        impl = mm.attrs.get("_impl")
        if impl is None or impl.n > 16 or impl.act != "none" or c.only_consumer(mm.name) is not sm:
            continue
        sm.op = "_DenseSoftmax"
        sm.inputs = [mm.inputs[0]]
        sm.ctrl = _merge_ctrl([mm, sm])
        sm.attrs = {"_impl": DenseSoftmax(impl)}
        del g.nodes[mm.name]
        c.refresh()


def _with_post(impl, y: torch.Tensor) -> list:
    """CPU reference of the post-activation output: [y] / [y, post] / [post]."""
    if impl.post is None:
        return [y]
    scale, shift, act = impl.post
    z = _ref_act(y * scale.to(y.device) + shift.to(y.device), act).contiguous()
    return [y, z] if impl.post_mode == "dual" else [z]


def _post_kwargs(impl, out: torch.Tensor):
    """(kernel kwargs, op outputs) for the fused post-activation output."""
    if impl.post is None:
        return {}, [out]
    from ..ops import ACT
    scale, shift, act = impl.post
    if impl.post_mode == "dual":
        out2 = torch.empty_like(out)
        return dict(post_scale=scale, post_shift=shift, post_act=ACT[act], out2=out2), [out, out2]
    return dict(post_scale=scale, post_shift=shift, post_act=ACT[act], post_only=True), [out]


def _ref_act(y, act):
    if act == "relu":
        return torch.relu(y)
    if act == "relu6":
        return torch.clamp(y, 0.0, 6.0)
    if act == "hard_sigmoid":
        return torch.clamp(y + 3.0, 0.0, 6.0) * (1.0 / 6.0)
    if act == "hard_swish":
        return y * (torch.clamp(y + 3.0, 0.0, 6.0) * (1.0 / 6.0))
    if act == "sigmoid":
        return torch.sigmoid(y)
    if act == "swish":
        return y * torch.sigmoid(y)
    if act == "tanh":
        return torch.tanh(y)
    if act == "gelu_tanh":
        return F.gelu(y, approximate="tanh")
    if act == "gelu_erf":
        return F.gelu(y)
    return y


def _impl_op(ctx, node, ins):
    return node.attrs["_impl"](ctx, node, ins)


for _op in ("_FusedConv2D", "_FusedDepthwiseConv2D", "_FusedDepthwiseLN", "_FusedGroupedConv2D", "_FusedDualConv", "_FusedMatMul", "_GlobalAvgPool", "_MaxPool",
            "_SqueezeExcite", "_SqueezeExciteSigmoid",
            "_SoftmaxArgMax", "_LayerNorm",
            "_FusedQKV", "_Attention", "_WindowAttention", "_EmbeddingLN", "_KeyMaskAdder", "_DenseSoftmax", "_PatchTokens",
            "_EmbeddingBag", "_DotInteraction"):
    O.OPS[_op] = _impl_op


class GlobalAvgPool:
    """``Mean`` over the axes the pass saw ({1, 2} or {-3, -2}).  Whether those
    are H and W of an NHWC tensor depends on the rank, which only the call
    knows: any other rank gets the Mean's own semantics from torch."""

    def __init__(self, keep_dims: bool, use_hip: bool, axes=(1, 2)):
        self.keep = keep_dims
        self.use_hip = use_hip
        self.axes = tuple(int(a) for a in axes)

    def __call__(self, ctx, node, ins):
        x = O.to_torch(ins[0])
        if x.dim() != 4 or sorted(a % 4 for a in self.axes) != [1, 2]:
            axes = sorted({a % x.dim() for a in self.axes})
            return [x.float().mean(dim=axes, keepdim=self.keep)]
        if self.use_hip and x.is_cuda and x.shape[-1] % 8 == 0:
            from ..ops import hip
            y = hip().global_avgpool(_to_bf16(x).contiguous())
        else:
            y = x.float().mean(dim=(1, 2))
        return [y.reshape(y.shape[0], 1, 1, -1) if self.keep else y]


class MaxPool(_Window):
    def __init__(self, ksize, strides, padding, use_hip, pads=(0, 0, 0, 0)):
        self._set_window(*ksize, strides, padding, tuple(pads))
        self.use_hip = use_hip
        self.post = None
        self.post_mode = None

    def set_post(self, scale, shift, act, mode, device=None):
        # on the device up front: a host->device copy inside HIP-graph capture is illegal
        dev = device if (self.use_hip and device is not None) else "cpu"
        self.post = (to_device(scale.float(), dev), to_device(shift.float(), dev), act)
        self.post_mode = mode

    def post_ok(self) -> bool:
        return True

    def __call__(self, ctx, node, ins):
        x = O.to_torch(ins[0])
        pt, pb, pl, pr = self.pads_for(x.shape[1], x.shape[2])
        if self.use_hip and x.is_cuda and x.shape[-1] % 8 == 0 and self.post_mode != "dual":
            from ..ops import ACT, hip
            kw = {}
            if self.post is not None:    # folded BN (+ReLU) after the max, same kernel
                sc, sh, act = self.post
                kw = dict(post_scale=sc, post_shift=sh, post_act=ACT[act])
            return [hip().maxpool(_to_bf16(x).contiguous(), self.kh, self.kw, self.sh, self.sw, pt, pb, pl, pr,
                                  **kw)]
        xc = F.pad(x.permute(0, 3, 1, 2), [pl, pr, pt, pb], value=float("-inf"))
        y = F.max_pool2d(xc, (self.kh, self.kw), (self.sh, self.sw)).permute(0, 2, 3, 1).contiguous()
        return _with_post(self, y)


class SoftmaxArgMax:
    """``Softmax(x)`` and ``ArgMax(x, axis)`` of the same x.  The pass sees the
    axis (1 or -1) but not the rank: where the axis is not the last one (axis 1
    of a rank-3 tensor) the classes come from torch, over that axis."""

    def __init__(self, use_hip, classes_dtype, axis=-1):
        self.use_hip = use_hip
        self.cdt = classes_dtype
        self.axis = int(axis)

    def __call__(self, ctx, node, ins):
        x = O.to_torch(ins[0])
        if x.dim() and self.axis % x.dim() != x.dim() - 1:
            probs = torch.softmax(x.float(), dim=-1)
            cls = torch.argmax(x.float(), dim=self.axis)
        elif self.use_hip and x.is_cuda and x.dim() == 2 and x.dtype in (torch.float32, BF16):
            from ..ops import hip
            if x.stride(-1) != 1:
                x = x.contiguous()
            probs, cls = hip().softmax_argmax(x, True, True)     # row-strided views are fine
        else:
            probs = torch.softmax(x.float(), dim=-1)
            cls = torch.argmax(x.float(), dim=-1)
        return [probs, cls if self.cdt == torch.int64 else cls.to(self.cdt)]


class ClassifierHead:
    """``_GlobalAvgPool -> _FusedMatMul (no act) -> _SoftmaxArgMax`` (the ResNet
    head) as two launches (``hip().classifier_head``: pooled split-K partial
    dot products, then bias + partial sums + softmax/argmax) instead of three
    with a 16-workgroup, 2048-deep serial GEMM in the middle."""

    def __init__(self, mm: FusedMatMul, classes_dtype, use_hip: bool, axes=(1, 2)):
        self.n, self.k = mm.n, mm.k
        self.axes = tuple(int(a) for a in axes)     # the Mean's own axes: H, W only at rank 4
        self.cdt = classes_dtype
        self.use_hip = use_hip and mm.use_hip and mm.k in (512, 1024, 2048, 4096)
        if mm.use_hip:
            self.w, self.b = mm.w, mm.b                     # bf16 [Np][K], f32 [Np]
        else:
            self.w_ref, self.b_ref = mm.w_ref, mm.b_ref     # f32 [K][N], [N]

    def __call__(self, ctx, node, ins):
        x = O.to_torch(ins[0])
        nhwc = x.dim() == 4 and sorted(a % 4 for a in self.axes) == [1, 2]
        if self.use_hip and x.is_cuda and nhwc and x.shape[-1] == self.w.shape[1]:
            from ..ops import current_head_host_rows, hip
            rows = current_head_host_rows()
            if rows is not None:
                # a serving lane's capture: the one-launch head also writes
                # the lane's pinned output rows (ops.head_host_rows)
                p_ptr = rows[0] if rows[1] == self.n else 0
                c_ptr = rows[2] if self.cdt == torch.int64 else 0
                probs, cls, wrote = hip().classifier_head_to_host(_to_bf16(x).contiguous(), self.w, self.b, self.n,
                                                                  p_ptr, c_ptr)
                if wrote:
                    probs._tfs_host, cls._tfs_host = p_ptr, c_ptr
                return [probs, cls]
            probs, cls = hip().classifier_head(_to_bf16(x).contiguous(), self.w, self.b, self.n)
        else:
            # (the Squeeze / Reshape between the pool and the GEMM gave it [rows, K] in row-major order)
            pooled = x.float().mean(dim=sorted({a % x.dim() for a in self.axes})).reshape(-1, self.k)
            if hasattr(self, "w_ref"):
                logits = pooled @ self.w_ref.to(x.device) + self.b_ref.to(x.device)
            else:
                logits = (pooled @ self.w.float().t().to(x.device) + self.b.to(x.device))[:, :self.n]
            probs = torch.softmax(logits, dim=-1)
            cls = torch.argmax(logits, dim=-1)
        return [probs, cls if self.cdt == torch.int64 else cls.to(self.cdt)]


O.OPS["_ClassifierHead"] = _impl_op


class StemPool:
    """``_FusedConv2D(7x7/2, RGB) -> _MaxPool(3x3/2)`` (the ResNet stem) as ONE
    kernel (``hip().stem_pool``, kernels/stem.hip): the fp32 request is read
    directly, the conv output stays in LDS and only the pooled map is written
    (three launches and two passes over the 112x112x64 conv output before)."""

    children = ("conv", "pool")        # weight_refs (graph/placement.py) walks these

    def __init__(self, conv: FusedConv, pool: MaxPool):
        self.conv, self.pool = conv, pool
        self.use_hip = conv.use_hip and conv.c4

    def accepts_bf16_input(self, pos: int) -> bool:
        """The kernel rounds the request to bf16 before its MFMAs: a request
        already rounded the same way on ingest gives identical results."""
        return pos == 0 and self.use_hip

    def __call__(self, ctx, node, ins):
        x = O.to_torch(ins[0])
        conv, pool = self.conv, self.pool
        if not (self.use_hip and x.is_cuda and x.dim() == 4):
            return pool(ctx, node, conv(ctx, node, [x]))
        from ..ops import ACT, hip
        pt, pb, pl, pr = conv.pads_for(x.shape[1], x.shape[2])
        hc, wc = conv.out_hw(x.shape[1], x.shape[2], (pt, pb, pl, pr))
        ppt, ppb, ppl, ppr = pool.pads_for(hc, wc)
        kw = {}
        if pool.post is not None:
            sc, sh, act = pool.post
            kw = dict(post_scale=sc, post_shift=sh, post_act=ACT[act])
        x = x.contiguous() if x.dtype == torch.bfloat16 else x.float().contiguous()
        return [hip().stem_pool(x, conv.w, conv.b, pt, pb, pl, pr, ACT[conv.act],
                                ppt, ppb, ppl, ppr, **kw)]


O.OPS["_StemPool"] = _impl_op

# (K1, N1, N2) shapes kernels/chain.hip is built for (ResNet-50 stages 1-2).
# Stage 2's (N1 = 512) pairs measured no faster chained than as two launches
# at b32 (each workgroup re-reads 256-384 KB of weights for 64 rows, one
# workgroup per CU: profiles/round3/conv_chain.md); since round 5 every shape
# is chained in the graph and ChainConv times the chain against the two
# convs per batch bucket (ops.tuned_choice), so each bucket runs its faster
# form.  TFSERVE_CONV_CHAIN_SHAPES=stage1 restores the stage-1-only pass.
#
# CHAIN_SHAPES_DUAL: (c1 + c2, N1, N2) of the dual form, where the expand is a
# stride-1 ``FusedDualConv`` (stage 1's projecting first block: expand conv
# and projection shortcut as one K-concatenated GEMM over two A sources).  A
# stage-1 shape: chained by default and kept by TFSERVE_CONV_CHAIN_SHAPES=stage1.
CHAIN_SHAPES_ALL = {(64, 256, 64), (64, 256, 128), (128, 512, 128), (128, 512, 256)}
CHAIN_SHAPES_STAGE1 = {(64, 256, 64), (64, 256, 128)}
CHAIN_SHAPES_DUAL = {(128, 256, 64)}
CHAIN_SHAPES_DEFAULT = CHAIN_SHAPES_ALL


class ChainConv:
    """A bottleneck's expand 1x1 conv (+ shortcut, act) and the NEXT
    bottleneck's reduce 1x1 conv (+ act), which reads exactly its output, as
    one kernel (``hip().conv_chain``, kernels/chain.hip): outputs
    ``[y1, y2]``; y1 (the block output, also the next shortcut) is written
    once and never read back by the reduce.  ``a`` is a ``FusedConv`` (inputs
    ``[x]`` or ``[x, residual]``) or a stride-1 ``FusedDualConv`` (inputs
    ``[h, x]``: the kernel's two A sources, no residual).  SURVEY.md S8 fused
    conv epilogues; the request path is the reference client's ResNet Predict
    (/root/reference/src/lib.rs:229-257)."""

    children = ("a", "b")

    def __init__(self, a, b: FusedConv):
        self.a, self.b = a, b
        self.dual = isinstance(a, FusedDualConv)
        self.use_hip = a.use_hip and b.use_hip
        self.name = a.name
        if self.dual:
            # three convs in one op (expand + projection shortcut + next
            # reduce): a flat op histogram (Program.op_histogram(flat=True),
            # which counts convs as 2 per dual conv and 2 per chain) lists the
            # two member ops, each of which runs as itself when the tuned
            # choice is 0; the plain histogram lists the _ChainConv
            from types import SimpleNamespace
            self.subs = [(a, SimpleNamespace(op="_FusedDualConv")), (b, SimpleNamespace(op="_FusedConv2D"))]

    def __call__(self, ctx, node, ins):
        x = O.to_torch(ins[0])
        a, b = self.a, self.b

        # the expand conv's own tuned choice (tile path or a row-panel form) is made first
        pp = a.panel_choice(ctx, node, ins) if isinstance(a, FusedConv) else None

        def split():
            y1 = (a(ctx, node, ins) if pp is None else a(ctx, node, ins, panel_pick=pp))[0]
            return [y1, b(ctx, node, [y1])[0]]
        if self.dual:
            return self._call_dual(x, O.to_torch(ins[1]), split)
        res = O.to_torch(ins[1]) if len(ins) > 1 else None
        if not (self.use_hip and x.is_cuda and x.dim() == 4 and x.shape[-1] == a.cin) or \
                (res is not None and tuple(res.shape) != tuple(x.shape[:3]) + (a.cout,)):
            return split()              # (a broadcast residual: the conv op expands it)
        from ..ops import ACT, hip, tuned_choice
        xb = _to_bf16(x).contiguous()
        rb = None if res is None else _to_bf16(res).contiguous()

        def chained():
            return list(hip().conv_chain(xb, a.w, a.b, rb, ACT[a.act], b.w, b.b, ACT[b.act]))
        # one workgroup per 64 rows: the chain wins where it saves a launch
        # boundary at small row counts or re-reads of large Y1 tiles, and loses
        # where 64-row workgroups leave CUs idle -- timed per shape (bucket):
        # option 1 = the chain kernel, 0 = the two convs with their own tiles
        key = ("chain", tuple(x.shape), a.cout, b.cout, res is not None, a.act, b.act)
        # without a tuned pick (TFSERVE_AUTOTUNE=0, no committed table, or a
        # key the table lacks) only the stage-1 shapes chain: the stage-2
        # (N1 = 512) chains measured no faster than two convs at b32
        # (round-5 ADVICE)
        dflt = 1 if (a.cin, a.cout, b.cout) in CHAIN_SHAPES_STAGE1 else 0
        pick = tuned_choice(key, {1: chained, 0: split}, default=dflt)
        return chained() if pick == 1 else split()

    def _call_dual(self, h, x, split):
        a, b = self.a, self.b
        if not (self.use_hip and h.is_cuda and h.dim() == 4 and x.dim() == 4 and h.shape[:3] == x.shape[:3] and
                h.shape[-1] == a.c1 and x.shape[-1] == a.c2):
            return split()
        from ..ops import ACT, hip, tuned_choice
        hb, xb = _to_bf16(h).contiguous(), _to_bf16(x).contiguous()

        def chained():
            return list(hip().conv_chain(hb, a.w, a.b, None, ACT[a.act], b.w, b.b, ACT[b.act], x2=xb))
        # the shortcut element (a plain chain's "has a residual" flag) names the
        # second source: this key differs from a plain chain's over the same h
        key = ("chain", tuple(h.shape), a.cout, b.cout, ("dual", a.c2), a.act, b.act)
        dflt = 1 if (a.c1 + a.c2, a.cout, b.cout) in CHAIN_SHAPES_DUAL else 0
        pick = tuned_choice(key, {1: chained, 0: split}, default=dflt)
        return chained() if pick == 1 else split()


O.OPS["_ChainConv"] = _impl_op
O.OPS["_FusedMatMulLN"] = _impl_op

_PASSTHROUGH = ("Identity", "Squeeze", "Reshape")


# ------------------------------------------------------------------ passes
def fuse_classifier_head(g, order, fed, fetch_refs, device, opts):
    """_SoftmaxArgMax(dense(mean_hw(x))) -> _ClassifierHead(x); every node in
    between must have that single consumer and not be fetched."""
    c = _Ctx(g, order, fed, fetch_refs, device, opts)

    def single(node) -> bool:
        return node.name not in c.fetch_nodes and len(c.cons.get(node.name, [])) == 1

    def walk(ref, chain):
        n = g.nodes.get(ref[0])
        while n is not None and n.op in _PASSTHROUGH and ref[1] == 0 and single(n) and n.inputs:
            chain.append(n)
            ref = n.inputs[0]
            n = g.nodes.get(ref[0])
        return ref, n

    def keeps_rows(nodes, cols) -> bool:
        """No Squeeze, and every Reshape is to [rows, cols]: the op in between sees the same rows."""
        for p in nodes:
            shp = _const(g, p.inputs[1]) if p.op == "Reshape" else None
            if p.op == "Squeeze" or (p.op == "Reshape" and
                                     (shp is None or shp.numel() != 2 or int(shp.reshape(-1)[1]) != cols)):
                return False
        return True

    for name in order:
        sm = g.nodes.get(name)
        if sm is None or sm.op != "_SoftmaxArgMax" or not sm.inputs:
            continue
        chain: List[Node] = []
        ref, mm = walk(sm.inputs[0], chain)
        if mm is None or mm.op != "_FusedMatMul" or ref[1] != 0 or len(mm.inputs) != 1 or not single(mm):
            continue
        impl = mm.attrs["_impl"]
        sm_impl = sm.attrs["_impl"]
        if impl.act != "none":
            continue
        if not keeps_rows(chain, impl.n):
            continue                  # the logits are regrouped before the softmax
        chain.append(mm)
        before = len(chain)
        ref, gap = walk(mm.inputs[0], chain)
        if gap is None or gap.op != "_GlobalAvgPool" or ref[1] != 0 or not single(gap):
            continue
        if not all(p.op != "Reshape" or keeps_rows([p], impl.k) for p in chain[before:]):
            continue
        gap_impl = gap.attrs["_impl"]
        chain.append(gap)
        head = ClassifierHead(impl, sm_impl.cdt, c.use_hip, gap_impl.axes)
        sm.op = "_ClassifierHead"
        sm.inputs = [gap.inputs[0]]
        sm.attrs = {"_impl": head}
        sm.ctrl = _merge_ctrl(chain + [sm])
        for n in chain:
            del g.nodes[n.name]
        c.refresh()


def fuse_stem_pool(g, order, fed, fetch_refs, device, opts):
    """``_MaxPool(3x3/2)(_FusedConv2D(7x7/2, C <= 4 channels, 16..64 outputs))``
    -> ``_StemPool`` when the conv has no residual / post output and feeds only
    the pool, and the pool writes a single output."""
    import os
    if os.environ.get("TFSERVE_STEM_POOL", "1") == "0":       # A/B switch
        return
    c = _Ctx(g, order, fed, fetch_refs, device, opts)
    for name in order:
        p = g.nodes.get(name)
        if p is None or p.op != "_MaxPool" or not p.inputs or p.inputs[0][1] != 0:
            continue
        pool = p.attrs["_impl"]
        if (pool.kh, pool.kw, pool.sh, pool.sw) != (3, 3, 2, 2) or pool.post_mode == "dual" or \
                pool.padding not in ("SAME", "VALID"):
            continue
        cn = g.nodes.get(p.inputs[0][0])
        if cn is None or cn.op != "_FusedConv2D" or len(cn.inputs) != 1 or c.only_consumer(cn.name) is not p:
            continue
        conv = cn.attrs["_impl"]
        if not isinstance(conv, FusedConv) or (conv.kh, conv.kw, conv.sh, conv.sw) != (7, 7, 2, 2) or \
                conv.cin > 4 or conv.cout % 16 or not 16 <= conv.cout <= 64 or conv.post is not None or \
                conv.act not in ("none", "relu"):
            continue
        if c.use_hip and not conv.c4:
            continue
        p.op = "_StemPool"
        p.inputs = [cn.inputs[0]]
        p.ctrl = _merge_ctrl([cn, p])
        p.attrs = {"_impl": StemPool(conv, pool)}
        del g.nodes[cn.name]
        c.refresh()


# ops whose output has the channel count of input 0 (NHWC pools included)
_SAME_CHANNELS = ("Identity", "StopGradient", "Snapshot", "Relu", "Relu6", "Elu", "Selu", "LeakyRelu", "Sigmoid",
                  "Tanh", "Softplus", "Neg", "Abs", "Square", "Sqrt", "Rsqrt", "Exp", "Cast", "_HardSwish",
                  "_HardSigmoid", "_SqueezeExcite", "_Swish", "_SqueezeExciteSigmoid", "MaxPool", "AvgPool", "_MaxPool")
_BATCH_NORMS = ("FusedBatchNorm", "FusedBatchNormV2", "FusedBatchNormV3")


def _channels_of(g: Graph, ref, fed=frozenset(), depth: int = 64, seen: Optional[Set] = None) -> Optional[int]:
    """The NHWC channel count (last dimension) of the value ``ref``, read off
    its producers' constants, or None.  The compiler infers no shapes and
    Conv2D has no ``groups`` attribute: this is how the passes tell a grouped
    conv from a dense one.  A count from here is what the graph declares; the
    fused ops still check the tensor they are given."""
    seen = set() if seen is None else seen
    n = g.nodes.get(ref[0])
    if n is None or depth <= 0 or ref in seen:
        return None
    seen.add(ref)
    if n.op == "Placeholder":
        shape = n.attrs.get("shape")
        return int(shape[-1]) if ref[1] == 0 and shape and len(shape) == 4 and shape[-1] > 0 else None
    if ref[0] in fed or ref[1] != 0:
        return None
    if n.op in ("_FusedConv2D", "_FusedGroupedConv2D", "_FusedDualConv"):
        return int(n.attrs["_impl"].cout)
    if n.op == "_FusedDepthwiseConv2D":
        return int(n.attrs["_impl"].c)
    nhwc = n.sattr("data_format", "NHWC") == "NHWC"
    if n.op in ("Conv2D", "DepthwiseConv2dNative") and nhwc:
        w = _const(g, n.inputs[1])
        if w is None or w.dim() != 4:
            return None
        return int(w.shape[3]) if n.op == "Conv2D" else int(w.shape[2] * w.shape[3])
    if (n.op in _BATCH_NORMS or n.op == "BiasAdd") and nhwc:
        v = _const(g, n.inputs[1])
        return int(v.numel()) if v is not None and v.dim() == 1 else None
    if n.op in _SAME_CHANNELS and nhwc and n.inputs:
        return _channels_of(g, n.inputs[0], fed, depth - 1, seen)
    if n.op == "Pad" and len(n.inputs) == 2:
        pv = _const(g, n.inputs[1])
        if pv is None or tuple(pv.shape) != (4, 2) or int(pv[3, 0]) or int(pv[3, 1]):
            return None
        return _channels_of(g, n.inputs[0], fed, depth - 1, seen)
    if n.op in ("Add", "AddV2", "Mul") and len(n.inputs) == 2:
        # whichever operand resolves; a 1 may be broadcast against the other operand
        got = {_channels_of(g, r, fed, depth - 1, seen) for r in n.inputs} - {None}
        wide = got - {1}
        return wide.pop() if len(wide) == 1 else None
    return None


def _absorb_pad(g: Graph, c: _Ctx, n: Node, x_ref, padding: str, pads, chain: List[Node]):
    """A spatial ``Pad`` in front of a VALID conv ``n`` (its only consumer)
    becomes the conv's explicit padding: (x_ref, padding, pads), the Pad
    appended to ``chain``."""
    prod = g.nodes.get(x_ref[0])
    if (padding == "VALID" and prod is not None and prod.op == "Pad" and x_ref[1] == 0
            and c.only_consumer(prod.name) is n):
        pv = _const(g, prod.inputs[1])
        if pv is not None:
            p = [int(v) for v in pv.reshape(-1).tolist()]
            if len(p) == 8 and p[0] == p[1] == p[6] == p[7] == 0 and min(p) >= 0:
                chain.append(prod)
                return prod.inputs[0], "EXPLICIT", (p[2], p[3], p[4], p[5])
    return x_ref, padding, pads


class _ConvChain:
    """What ``_match_conv_chain`` found: the conv's input and padding, the fp32
    filter and bias with everything so far folded in, and a cursor -- the nodes
    taken (``chain``, which ``_finalize`` deletes) and the node at the end
    (``cur``).  The passes move the cursor on over what only they absorb."""

    def __init__(self, c: _Ctx, x_ref, padding: str, pads, strides, w, bias, chain: List[Node]):
        self.c, self.x_ref, self.padding, self.pads, self.strides = c, x_ref, padding, pads, strides
        self.w, self.bias, self.act = w, bias, "none"
        self.chain, self.cur = chain, chain[-1]

    @property
    def nxt(self) -> Optional[Node]:
        """The only reader of output 0 of ``cur``, when ``cur`` is not fetched."""
        return self.c.only_consumer(self.cur.name)

    def take(self, *nodes: Node) -> Optional[Node]:
        """Append ``nodes`` (the last one is the new ``cur``); returns the new ``nxt``."""
        self.chain += nodes
        self.cur = nodes[-1]
        return self.nxt

    def close(self, acts: Dict[str, str]):
        """Take ``nxt`` as the closing activation if its op is one of ``acts`` (op -> the kernels' name)."""
        nxt = self.nxt
        if nxt is not None and nxt.op in acts:
            self.act = acts[nxt.op]
            self.take(nxt)


def _match_conv_chain(g: Graph, c: _Ctx, n: Node, accept) -> Optional[_ConvChain]:
    """The head the conv passes share, from the ``Conv2D`` / ``DepthwiseConv2dNative``
    node ``n``: ``[Pad ->] n [-> BiasAdd] [-> FusedBatchNorm*]``, or None.

    Guards: NHWC, dilation 1, a constant 4-D filter, ``EXPLICIT`` paddings with
    zero batch and channel entries.  ``accept(filter)`` holds the calling pass's
    own conditions: it returns the filter as the pass's op takes it, output
    channels last, or None to leave the conv alone.  A spatial ``Pad`` read only
    by ``n`` becomes explicit padding; a ``BiasAdd`` of a constant ``(cout,)``
    and an inference BatchNorm with ``cout`` elements (``_bn_affine``) are folded
    as ``w *= scale; bias = bias * scale + shift`` -- tensor arithmetic only, so
    that shape-only (meta) weights fold too."""
    if n.sattr("data_format", "NHWC") != "NHWC":
        return None
    dil = n.attr("dilations", [1, 1, 1, 1]) or [1, 1, 1, 1]
    if any(d != 1 for d in dil):
        return None
    w = _const(g, n.inputs[1])
    w = accept(w) if w is not None and w.dim() == 4 else None
    if w is None:
        return None
    padding = n.sattr("padding", "VALID")
    pads = (0, 0, 0, 0)
    chain: List[Node] = []
    if padding == "EXPLICIT":
        ep = n.attr("explicit_paddings", [])
        if ep[0] or ep[1] or ep[6] or ep[7]:
            return None
        pads = (ep[2], ep[3], ep[4], ep[5])
    x_ref, padding, pads = _absorb_pad(g, c, n, n.inputs[0], padding, pads, chain)
    strides = n.attr("strides", [1, 1, 1, 1])
    w = w.float()
    cout = w.shape[-1]
    m = _ConvChain(c, x_ref, padding, pads, (strides[1], strides[2]), w, zeros(cout, w), chain + [n])
    nxt = m.nxt
    if nxt is not None and nxt.op == "BiasAdd" and nxt.inputs[0] == (m.cur.name, 0):
        b = _const(g, nxt.inputs[1])
        if b is not None and tuple(b.shape) == (cout,):
            m.bias = m.bias + b.float()
            nxt = m.take(nxt)
    if nxt is not None and nxt.op in _BATCH_NORMS and nxt.inputs[0] == (m.cur.name, 0):
        aff = _bn_affine(g, c, nxt)
        if aff is not None and aff[0].numel() == cout:
            m.w = m.w * aff[0]
            m.bias = m.bias * aff[0] + aff[1]
            m.take(nxt)
    return m


def _bn_affine(g: Graph, c: _Ctx, bn: Node):
    """(scale, shift) of an inference FusedBatchNorm with constant params whose
    only used output is y, else None."""
    if bn.op not in _BATCH_NORMS or bn.attr("is_training", False) \
            or bn.sattr("data_format", "NHWC") != "NHWC" or bn.name in c.fetch_nodes:
        return None
    params = [_const(g, r) for r in bn.inputs[1:5]]
    if any(p is None for p in params) or {i for _c, _p, i in c.cons.get(bn.name, [])} - {0}:
        return None
    gamma, beta, mean, var = (p.float().reshape(-1) for p in params)
    scale = gamma * torch.rsqrt(var + float(bn.attr("epsilon", 1e-3)))
    return scale, beta - mean * scale


def _group_channels(g: Graph, n: Node, fed, w: torch.Tensor) -> Optional[int]:
    """The input channel count the graph declares for ``Conv2D`` ``n`` where it
    makes ``n`` a grouped conv -- a proper multiple of the filter's in-depth,
    which is above 1, with the outputs dividing among the groups -- else None."""
    cg, cout = int(w.shape[2]), int(w.shape[3])
    ch = _channels_of(g, n.inputs[0], fed) if cg > 1 else None
    return None if ch is None or ch == cg or ch % cg or cout % (ch // cg) else ch


def fuse_grouped_conv(g, order, fed, fetch_refs, device, opts):
    """``[Pad ->] Conv2D [-> BiasAdd] [-> FusedBatchNorm*] [-> Relu]`` ->
    ``_FusedGroupedConv2D`` where the conv is a GROUPED one: the channel count
    of its input (``_channels_of``) is known and a proper multiple of the
    filter's in-depth, which is above 1 (in-depth 1 is a depthwise conv spelled
    as Conv2D: it stays on the reference op).  ``_match_conv_chain``'s guards apply
    (NHWC, dilation 1, a constant 4-D filter, an inference BatchNorm whose only used
    output is y, no fetch inside the chain, single consumers).  No residual
    ``Add`` is absorbed (the kernel reads none), and a closing activation other
    than Relu stays a node of its own.  3x3 filters with 4 / 8 / 16 / 32
    inputs and outputs per group run kernels/gconv.hip on the GPU, any other
    shape torch's grouped conv on the device.

    Runs directly before fuse_conv, which skips what this pass left for the
    same reason (a known channel count that differs from the in-depth).  The
    later passes (fuse_dual_conv, fuse_post_activation, fuse_stem_pool,
    fuse_conv_chain, the late passes) look for ``_FusedConv2D`` by op name, so
    ``_FusedGroupedConv2D`` is opaque to them: it is never a dual-conv half, a
    post-activation producer or a chain link."""
    c = _Ctx(g, order, fed, fetch_refs, device, opts)
    for name in order:
        n = g.nodes.get(name)
        if n is None or n.op != "Conv2D":
            continue
        m = _match_conv_chain(g, c, n, lambda w: w if _group_channels(g, n, fed, w) else None)
        if m is None:
            continue
        m.close({"Relu": "relu"})
        impl = FusedGroupedConv(m.w, m.bias, m.strides, m.padding, m.pads, m.act, device, c.use_hip, m.cur.name,
                                _group_channels(g, n, fed, m.w))
        _finalize(g, m.chain, "_FusedGroupedConv2D", [m.x_ref], {"_impl": impl})
        c.refresh()


def fuse_conv(g, order, fed, fetch_refs, device, opts):
    """``_match_conv_chain``'s head ``[-> Mul(const [C])] [-> Add(residual)] [-> GELU subgraph | Relu | Relu6 |
    _HardSwish | _Swish]`` -> ``_FusedConv2D`` for a dense ``Conv2D``."""
    c = _Ctx(g, order, fed, fetch_refs, device, opts)
    for name in order:
        n = g.nodes.get(name)
        if n is None or n.op != "Conv2D":
            continue

        def dense(w):
            # a grouped conv (Conv2D has no groups attribute: its input has more channels than the filter's
            # in-depth) is fuse_grouped_conv's, or stays on the reference op; an input whose channel count
            # the graph does not tell is checked by FusedConv when it runs
            return w if _channels_of(g, n.inputs[0], fed) in (None, int(w.shape[2])) else None
        m = _match_conv_chain(g, c, n, dense)
        if m is None:
            continue
        cout = m.w.shape[3]
        residual = None
        nxt = m.nxt
        # a constant per-channel / scalar scale (ResNet v2's residual scale):
        # folded into the weights and bias
        if nxt is not None and nxt.op == "Mul" and len(nxt.inputs) == 2 and (m.cur.name, 0) in nxt.inputs:
            other = _other(nxt, (m.cur.name, 0))
            # by shape, not by size: [C], [1,1,1,C] or one element (a [C,1] constant scales along W)
            sv = _channel_const(_const(g, other), cout, 4)
            if sv is not None and other != (m.cur.name, 0):
                m.w = m.w * sv
                m.bias = m.bias * sv
                nxt = m.take(nxt)
        if nxt is not None and nxt.op in ("Add", "AddV2") and len(nxt.inputs) == 2:
            other = _other(nxt, (m.cur.name, 0))
            if other != (m.cur.name, 0) and _const(g, other) is None:
                residual = other
                nxt = m.take(nxt)
        # a GELU subgraph (erf or tanh form) closes the chain like a one-node activation: after the
        # residual add, which is the order of the kernels' epilogue
        gelu = match_gelu(g, c, m.cur.name)
        if gelu is not None:
            m.act, gnodes, out_node = gelu
            m.take(*gnodes, out_node)
        else:
            m.close(_CLOSING_ACTS)
        impl = FusedConv(m.w, m.bias, m.strides, m.padding, m.pads, m.act, device, c.use_hip, m.cur.name)
        inputs = [m.x_ref] + ([residual] if residual is not None else [])
        _finalize(g, m.chain, "_FusedConv2D", inputs, {"_impl": impl})
        c.refresh()


def fuse_depthwise(g, order, fed, fetch_refs, device, opts):
    """``[Pad ->] DepthwiseConv2dNative [-> BiasAdd] [-> FusedBatchNorm*] [-> Relu | Relu6 | _HardSwish | _Swish]``
    -> ``_FusedDepthwiseConv2D``, under ``_match_conv_chain``'s guards (NHWC,
    dilation 1, a constant 4-D filter, an inference BatchNorm whose only used
    output is y, no fetch inside the chain, single consumers) and channel
    multiplier 1.  On the GPU also C % 8 == 0 and a filter of at most 7 x 7
    (kernels/dwconv.hip); anything else stays on the reference op."""
    c = _Ctx(g, order, fed, fetch_refs, device, opts)

    def multiplier_1(w):
        """The [kh, kw, ch, 1] filter as the op's [kh, kw, ch]."""
        kh, kw, ch, mult = w.shape
        return w.reshape(kh, kw, ch) if mult == 1 and (not c.use_hip or FusedDepthwiseConv.hip_ok(kh, kw, ch)) \
            else None
    for name in order:
        n = g.nodes.get(name)
        if n is None or n.op != "DepthwiseConv2dNative":
            continue
        m = _match_conv_chain(g, c, n, multiplier_1)
        if m is None:
            continue
        m.close(_CLOSING_ACTS)
        impl =FusedDepthwiseConv(m.w, m.bias, m.strides, m.padding, m.pads, m.act, device, c.use_hip, m.cur.name)
        _finalize(g, m.chain, "_FusedDepthwiseConv2D", [m.x_ref], {"_impl": impl})
        c.refresh()


def fuse_depthwise_layernorm(g, order, fed, fetch_refs, device, opts):
    """``_LayerNorm(_FusedDepthwiseConv2D(x))`` -> ``_FusedDepthwiseLN`` (the
    opening of a ConvNeXt block) when the depthwise op is 7 x 7 / stride 1
    without activation, the LayerNorm is its only reader, it is not fetched, and
    gamma and beta have C elements or one each.  On the GPU also what
    kernels/dwln.hip takes (C % 8 == 0, 8 <= C <= kDwLnMaxC).  Runs after
    fuse_layernorm and fuse_depthwise; ``TFSERVE_DWLN=0`` keeps the pair."""
    if os.environ.get("TFSERVE_DWLN", "1") == "0":
        return
    c = _Ctx(g, order, fed, fetch_refs, device, opts)
    for name in order:
        n = g.nodes.get(name)
        if n is None or n.op != "_FusedDepthwiseConv2D":
            continue
        dw = n.attrs["_impl"]
        if not FusedDepthwiseLN.shape_ok(dw):
            continue
        ln = c.only_consumer(name)
        if ln is None or ln.op != "_LayerNorm" or ln.inputs != [(name, 0)]:
            continue
        limpl = ln.attrs["_impl"]
        if any(v.numel() not in (1, dw.c) for v in (limpl.g, limpl.b)):
            continue
        if c.use_hip:
            from ..ops import hip
            if not hip().dwconv_ln_supported(1, 1, 1, dw.c, dw.kh, dw.kw, dw.sh, dw.sw):
                continue
        impl = FusedDepthwiseLN(dw, limpl, c.use_hip, ln.name)
        _finalize(g, [n, ln], "_FusedDepthwiseLN", list(n.inputs), {"_impl": impl})
        c.refresh()


# ------------------------------------------------------------------ ViT patch tokens
class PatchTokens:
    """``AddV2(ConcatV2([cls_b, Reshape(x, [-1, P, C])], axis=1), pos)`` with
    ``cls_b`` the ``[1, 1, C]`` class token repeated ``batch`` times (the op's
    second input: the graph's own ``Shape -> StridedSlice`` scalar).  The pass
    sees constants only; whether ``x`` is the patch conv's ``[B, H, W, C]``
    output with ``H * W == P`` is known at the call.  Then, on the GPU, one
    ``patch_tokens`` launch from the fp32 table (row 0 = class token + pos[0],
    rows 1.. = pos[1..]); any other input, and the CPU, gets the replaced
    nodes' own semantics from torch."""

    def __init__(self, cls: torch.Tensor, pos: torch.Tensor, p: int, c: int, device, use_hip: bool, name: str):
        self.p, self.c = int(p), int(c)
        self.use_hip = use_hip
        self.name = name
        self.cls = to_device(cls.float().reshape(1, 1, self.c), device)
        self.pos = to_device(pos.float().reshape(self.p + 1, self.c), device)
        self.pos_rank = pos.dim()
        table = pos.float().reshape(self.p + 1, self.c).clone()
        if not table.is_meta:
            table[0] += cls.float().reshape(self.c)
        self.table = to_device(table, device) if use_hip else None

    def __call__(self, ctx, node, ins):
        x = O.to_torch(ins[0])
        batch = O.host_int(ins[1])
        P, C = self.p, self.c
        if (self.use_hip and x.is_cuda and x.dim() == 4 and x.shape[1] * x.shape[2] == P and x.shape[3] == C
                and x.shape[0] == batch):
            from ..ops import hip
            H = hip()
            if H.patch_tokens_supported(batch, P, C):
                return [H.patch_tokens(_to_bf16(x).contiguous().view(batch, P, C), self.table)]
        try:
            r = x.reshape(-1, P, C)
        except RuntimeError as e:
            raise O.OpError(f"{node.name}: cannot reshape {list(x.shape)} to [-1, {P}, {C}]: {e}") from None
        cls, pos = self.cls.to(x.device), self.pos.to(x.device)
        y = torch.cat([cls.repeat(batch, 1, 1), r.float()], dim=1) + (pos if self.pos_rank == 2 else pos.unsqueeze(0))
        return [y.to(x.dtype) if x.is_cuda and x.dtype == BF16 else y]


def _batch_scalar(g: Graph, ref) -> bool:
    """``ref`` = StridedSlice(Shape(.), ..): a run-time scalar of the graph's own."""
    ss = g.nodes.get(ref[0])
    if ss is None or ref[1] != 0 or ss.op != "StridedSlice" or not ss.inputs:
        return False
    sh = g.nodes.get(ss.inputs[0][0])
    return sh is not None and sh.op == "Shape"


def _repeated_token(g: Graph, ref, c_hint=None):
    """``ref`` = Tile(cls[1, 1, C], Pack([batch, 1, 1])) or BroadcastTo(cls[1, 1, C],
    Pack([batch, 1, C])) -> (cls, batch ref, [rep, pack]) or None."""
    rep = g.nodes.get(ref[0])
    if rep is None or ref[1] != 0 or rep.op not in ("Tile", "BroadcastTo") or len(rep.inputs) != 2:
        return None
    cls = _const(g, rep.inputs[0])
    pack = g.nodes.get(rep.inputs[1][0])
    if cls is None or cls.dim() != 3 or cls.shape[0] != 1 or cls.shape[1] != 1 or not cls.is_floating_point():
        return None
    if pack is None or rep.inputs[1][1] != 0 or pack.op != "Pack" or len(pack.inputs) != 3 or \
            int(pack.attr("axis", 0)) != 0:
        return None
    if not _batch_scalar(g, pack.inputs[0]):
        return None
    want = (1, 1) if rep.op == "Tile" else (1, int(cls.shape[2]))
    for r, w in zip(pack.inputs[1:], want):
        v = _const(g, r)
        if v is None or v.numel() != 1 or v.dim() != 0 or int(v) != w:
            return None
    return cls, pack.inputs[0], [rep, pack]


def fuse_patch_tokens(g, order, fed, fetch_refs, device, opts):
    """The front of a ViT behind its patch conv ->  ``_PatchTokens(x, batch)``
    (class PatchTokens has the pattern).  Matched by shape: the class token is
    ``[1, 1, C]``, the reshape's target ``[-1, P, C]``, the concat on axis 1
    with the token first, ``pos`` a ``[1, P + 1, C]`` or ``[P + 1, C]``
    constant on either side of the add.  The concat, the reshape, the repeat
    and its Pack must be read inside the pattern only and not be fetched.
    Runs after fuse_conv, so ``x`` is the fused conv's output."""
    c = _Ctx(g, order, fed, fetch_refs, device, opts)
    for name in order:
        add = g.nodes.get(name)
        if add is None or add.op not in ("Add", "AddV2") or len(add.inputs) != 2:
            continue
        for cat_ref, pos_ref in ((add.inputs[0], add.inputs[1]), (add.inputs[1], add.inputs[0])):
            cat = g.nodes.get(cat_ref[0])
            pos = _const(g, pos_ref)
            if cat is None or cat_ref[1] != 0 or cat.op != "ConcatV2" or len(cat.inputs) != 3 or pos is None:
                continue
            axis = _const(g, cat.inputs[2])
            if axis is None or axis.numel() != 1 or int(axis.reshape(-1)[0]) != 1:
                continue
            tok = _repeated_token(g, cat.inputs[0])
            rs = g.nodes.get(cat.inputs[1][0])
            if tok is None or rs is None or cat.inputs[1][1] != 0 or rs.op != "Reshape":
                continue
            cls, batch_ref, rep_nodes = tok
            shp = _const(g, rs.inputs[1])
            if shp is None or shp.numel() != 3:
                continue
            lead, P, C = [int(v) for v in shp.reshape(-1).tolist()]
            if lead != -1 or P < 1 or C != int(cls.shape[2]) or not pos.is_floating_point():
                continue
            if tuple(pos.shape) not in ((1, P + 1, C), (P + 1, C)):
                continue
            interior = [cat, rs] + rep_nodes
            names = {n.name for n in interior} | {add.name}
            if any(n.name in c.fetch_nodes or any(cn not in names for cn, _p, _i in c.cons.get(n.name, []))
                   for n in interior):
                continue
            # each inner value read once: the concat by the add, the reshape and the repeat by the concat
            if any(len(c.cons.get(n.name, [])) != 1 for n in interior):
                continue
            impl = PatchTokens(cls, pos, P, C, device, c.use_hip, add.name)
            ctrl = _merge_ctrl(interior + [add])
            for n in interior:
                del g.nodes[n.name]
            add.op = "_PatchTokens"
            add.inputs = [rs.inputs[0], batch_ref]
            add.ctrl = ctrl
            add.attrs = {"_impl": impl}
            add.value = None
            c.refresh()
            break


# ------------------------------------------------------------------ hard activations (MobileNetV3)
def _hard_sigmoid_op(ctx, node, ins):
    """clamp(x + 3, 0, 6) * c with the graph's own c (1/6 within 1e-4), in the
    order the unfused nodes computed it."""
    x = O.to_torch(ins[0])
    y = torch.clamp(x.float() + 3.0, 0.0, 6.0) * float(node.attr("scale", 1.0 / 6.0))
    return [y.to(x.dtype) if x.dtype == BF16 else y]


def _hard_swish_op(ctx, node, ins):
    x = O.to_torch(ins[0])
    xf = x.float()
    y = xf * (torch.clamp(xf + 3.0, 0.0, 6.0) * float(node.attr("scale", 1.0 / 6.0)))
    return [y.to(x.dtype) if x.dtype == BF16 else y]


O.OPS["_HardSigmoid"] = _hard_sigmoid_op
O.OPS["_HardSwish"] = _hard_swish_op


def _one_element(g: Graph, ref, want: float, rel: float) -> Optional[float]:
    """The value of a one-element floating constant (a scalar or a [1]: by
    shape, a [C] constant of equal entries is not one) within ``rel`` of
    ``want``, else None."""
    v = _const(g, ref)
    if v is None or v.numel() != 1 or v.dim() > 1 or not v.is_floating_point():
        return None
    f = float(v.reshape(-1)[0])
    return f if abs(f - want) <= rel * abs(want) else None


def _other(node: Node, ref):
    """The other input of a two-input node one of whose inputs is ``ref``."""
    if len(node.inputs) != 2 or ref not in node.inputs:
        return None
    return node.inputs[1] if node.inputs[0] == ref else node.inputs[0]


def _relu6_of_x_plus_3(g: Graph, c: _Ctx, ref, reader: Node):
    """``ref`` = Relu6(Add|AddV2(x, 3)) read by ``reader`` alone -> (x, [add, relu6]) or None."""
    r = g.nodes.get(ref[0])
    if r is None or ref[1] != 0 or r.op != "Relu6" or len(r.inputs) != 1 or c.only_consumer(r.name) is not reader:
        return None
    a = g.nodes.get(r.inputs[0][0])
    if a is None or r.inputs[0][1] != 0 or a.op not in ("Add", "AddV2") or len(a.inputs) != 2 or \
            c.only_consumer(a.name) is not r:
        return None
    for x_ref, k_ref in ((a.inputs[0], a.inputs[1]), (a.inputs[1], a.inputs[0])):
        if _one_element(g, k_ref, 3.0, 1e-6) is not None and _const(g, x_ref) is None:
            return x_ref, [a, r]
    return None


HARD_SCALE_REL = 1e-4       # slim writes 0.16667 for 1/6 (2e-5 off); docs/numerics.md


def fuse_hard_activations(g, order, fed, fetch_refs, device, opts):
    """``Mul(Relu6(Add|AddV2(x, 3)), c)`` -> ``_HardSigmoid(x)``;
    ``Mul(x, _HardSigmoid(x))`` and the slim association ``Mul(Mul(x,
    Relu6(Add(x, 3))), c)`` -> ``_HardSwish(x)``.  Operands in either order; 3
    and c one-element constants, c within 1e-4 of 1/6 (kept on the node: the
    standalone op multiplies by it); inner nodes read once and not fetched;
    x may have other readers."""
    c = _Ctx(g, order, fed, fetch_refs, device, opts)
    for name in order:
        m = g.nodes.get(name)
        if m is None or m.op != "Mul" or len(m.inputs) != 2:
            continue
        for inner_ref, k_ref in ((m.inputs[0], m.inputs[1]), (m.inputs[1], m.inputs[0])):
            scale = _one_element(g, k_ref, 1.0 / 6.0, HARD_SCALE_REL)
            if scale is None:
                continue
            hit = _relu6_of_x_plus_3(g, c, inner_ref, m)
            if hit is not None:
                x_ref, inner = hit
                _finalize(g, inner + [m], "_HardSigmoid", [x_ref], {"scale": scale})
                c.refresh()
                break
            # slim: the outer Mul scales Mul(x, Relu6(x + 3))
            i = g.nodes.get(inner_ref[0])
            if i is None or inner_ref[1] != 0 or i.op != "Mul" or len(i.inputs) != 2 or c.only_consumer(i.name) is not m:
                continue
            for x_ref, r_ref in ((i.inputs[0], i.inputs[1]), (i.inputs[1], i.inputs[0])):
                hit = _relu6_of_x_plus_3(g, c, r_ref, i)
                if hit is not None and hit[0] == x_ref:
                    _finalize(g, hit[1] + [i, m], "_HardSwish", [x_ref], {"scale": scale})
                    c.refresh()
                    break
            if m.op != "Mul":
                break
    for name in order:
        m = g.nodes.get(name)
        if m is None or m.op != "Mul" or len(m.inputs) != 2:
            continue
        for x_ref, s_ref in ((m.inputs[0], m.inputs[1]), (m.inputs[1], m.inputs[0])):
            s = g.nodes.get(s_ref[0])
            if s is None or s_ref[1] != 0 or s.op != "_HardSigmoid" or s.inputs[0] != x_ref or \
                    c.only_consumer(s.name) is not m:
                continue
            _finalize(g, [s, m], "_HardSwish", [x_ref], {"scale": s.attr("scale", 1.0 / 6.0)})
            c.refresh()
            break



# ------------------------------------------------------------------ swish (EfficientNet)
def _swish_op(ctx, node, ins):
    x = O.to_torch(ins[0])
    xf = x.float()
    y = xf * torch.sigmoid(xf)
    return [y.to(x.dtype) if x.dtype == BF16 else y]


O.OPS["_Swish"] = _swish_op


def fuse_swish(g, order, fed, fetch_refs, device, opts):
    """``Mul(x, Sigmoid(x))`` and ``Mul(x, Sigmoid(Mul(x, b)))`` with ``b`` a
    one-element constant exactly 1.0 (TF >= 2.4's swish_impl) -> ``_Swish(x)``;
    and either one read through output 0 of an ``IdentityN`` whose input 0 is
    that Mul and whose other outputs have no reader and are not fetched (the
    custom_gradient wrapper).  fuse_hard_activations' rules: operands in either
    order, inner nodes read once and not fetched; x may have other readers."""
    c = _Ctx(g, order, fed, fetch_refs, device, opts)
    for name in order:
        m = g.nodes.get(name)
        if m is None or m.op != "Mul" or len(m.inputs) != 2:
            continue
        for x_ref, s_ref in ((m.inputs[0], m.inputs[1]), (m.inputs[1], m.inputs[0])):
            s = g.nodes.get(s_ref[0])
            if s is None or s_ref[1] != 0 or s.op != "Sigmoid" or len(s.inputs) != 1 or \
                    c.only_consumer(s.name) is not m or _const(g, x_ref) is not None:
                continue
            inner = [s]
            if s.inputs[0] != x_ref:
                b = g.nodes.get(s.inputs[0][0])
                if b is None or s.inputs[0][1] != 0 or b.op != "Mul" or len(b.inputs) != 2 or \
                        c.only_consumer(b.name) is not s:
                    continue
                k_ref = _other(b, x_ref)
                if k_ref is None or k_ref == x_ref or _one_element(g, k_ref, 1.0, 0.0) is None:
                    continue
                inner = [b, s]
            chain = inner + [m]
            idn = c.only_consumer(m.name)
            if idn is not None and idn.op == "IdentityN" and idn.inputs and idn.inputs[0] == (m.name, 0) and \
                    all(r != (m.name, 0) for r in idn.inputs[1:]):
                readers = c.cons.get(idn.name, [])
                if not all(oidx == 0 for _n, _p, oidx in readers) or \
                        any(fn == idn.name and fi != 0 for fn, fi in c.fetch_refs):
                    continue          # a wrapper whose other outputs are in use is left as it is, swish and all
                chain.append(idn)
            _finalize(g, chain, "_Swish", [x_ref], {})
            c.refresh()
            break

# ------------------------------------------------------------------ squeeze-and-excite
class SqueezeExcite:
    """``x * gate(act1(mean_hw(x) w1 + b1) w2 + b2)`` with the gate broadcast
    over H and W; ``gate`` is "hard_sigmoid" (``_SqueezeExcite``, MobileNetV3) or
    "sigmoid" (``_SqueezeExciteSigmoid``, EfficientNet: ``torch.sigmoid`` on the
    reference path, ``scale`` unused).  w1 [C][Cr], w2 [Cr][C]: the TF 1x1 filters reshaped
    [Cin][Cout]; they and the biases stay fp32 on both paths.  On the GPU two
    launches, ``se_gate`` then ``se_scale`` (kernels/se.hip), which use 1/6 for
    the gate's scale; the reference path multiplies by the graph's constant.
    What depends on the rank is decided per call: an ``x`` that is not rank 4
    gets the original nodes' semantics from torch."""

    def __init__(self, w1, b1, w2, b2, act1: str, scale: float, keep_dims: bool, axes, reshape, device, use_hip: bool,
                 name: str, gate: str = "hard_sigmoid"):
        self.c, self.cr = w1.shape
        self.act1 = act1
        self.gate = gate
        self.scale = float(scale)
        self.keep = keep_dims
        self.axes = tuple(int(a) for a in axes)
        self.reshape = None if reshape is None else [int(v) for v in reshape]
        self.use_hip = use_hip
        self.name = name
        self.device = device
        self.w1 = to_device(w1.float().contiguous(), device)
        self.b1 = to_device(b1.float().contiguous(), device)
        self.w2 = to_device(w2.float().contiguous(), device)
        self.b2 = to_device(b2.float().contiguous(), device)
        # se_gate masks its idle FC lanes by feeding 0 to an FMA against a real weight: an Inf / NaN
        # weight would reach gates it has no part in, so such a model keeps the torch path
        if self.use_hip and not all(t.is_meta or bool(torch.isfinite(t).all()) for t in (w1, b1, w2, b2)):
            self.use_hip = False

    def _params(self, dev):
        return (t.to(dev) for t in (self.w1, self.b1, self.w2, self.b2))

    def _gate(self, z):
        if self.gate == "sigmoid":
            return torch.sigmoid(z)
        return torch.clamp(z + 3.0, 0.0, 6.0) * self.scale

    def _original(self, x):
        """The matched nodes one by one (Mean, [Reshape], Conv2D + bias, act1,
        Conv2D + bias, hard-sigmoid, Mul) for an x the kernels do not take."""
        w1, b1, w2, b2 = self._params(x.device)
        xf = x.float()
        p = xf.mean(dim=sorted({a % x.dim() for a in self.axes}), keepdim=self.keep)
        if self.reshape is not None:
            p = p.reshape(self.reshape)

        def conv1x1(t, w):
            return F.conv2d(t.permute(0, 3, 1, 2), w.t().reshape(w.shape[1], w.shape[0], 1, 1)).permute(0, 2, 3, 1)
        h = _ref_act(conv1x1(p, w1) + b1, self.act1)
        return xf * self._gate(conv1x1(h, w2) + b2)

    def __call__(self, ctx, node, ins):
        x = O.to_torch(ins[0])
        if x.dim() != 4 or x.shape[3] != self.c:
            y = self._original(x)
            return [y.to(BF16) if x.dtype == BF16 else y]
        if self.use_hip and x.is_cuda:
            from ..ops import ACT, hip
            H = hip()
            if H.se_gate_supported(x.shape[0], x.shape[1] * x.shape[2], self.c, self.cr) and x.numel() > 0:
                xb = _to_bf16(x).contiguous()
                gate = H.se_gate(xb, self.w1, self.b1, self.w2, self.b2, ACT[self.act1], ACT[self.gate])
                return [H.se_scale(xb, gate)]
        w1, b1, w2, b2 = self._params(x.device)
        xf = x.float()
        h = _ref_act(xf.mean(dim=(1, 2)) @ w1 + b1, self.act1)
        y = xf * self._gate(h @ w2 + b2)[:, None, None, :]
        return [y.to(BF16) if x.dtype == BF16 else y]


def _fc_1x1(g: Graph, n: Optional[Node]):
    """A Conv2D that is a per-pixel FC (1x1, stride 1, dilation 1, NHWC, no
    padding, constant 4-D filter) -> its [Cin][Cout] fp32 weight, else None."""
    if n is None or n.op != "Conv2D" or len(n.inputs) != 2 or n.sattr("data_format", "NHWC") != "NHWC":
        return None
    if any(v != 1 for v in (n.attr("dilations", [1, 1, 1, 1]) or [1, 1, 1, 1])) or \
            any(v != 1 for v in n.attr("strides", [1, 1, 1, 1])) or n.sattr("padding", "VALID") not in ("SAME", "VALID"):
        return None
    w = _const(g, n.inputs[1])
    if w is None or w.dim() != 4 or w.shape[0] != 1 or w.shape[1] != 1:
        return None
    return w.float().reshape(w.shape[2], w.shape[3])


def fuse_squeeze_excite(g, order, fed, fetch_refs, device, opts):
    """``Mul(x, g)`` / ``Mul(g, x)`` with ``g = _HardSigmoid([BiasAdd](Conv2D_2(
    [Relu]([BiasAdd](Conv2D_1(pool(x)))))))`` -> ``_SqueezeExcite(x)``.  ``pool``
    is a ``_GlobalAvgPool`` over H, W of the very ``x`` being multiplied, with
    keep_dims, or without and followed by a Reshape to [-1, 1, 1, C]; both
    convs are per-pixel FCs (``_fc_1x1``) of matching C -> Cr -> C; every node
    of the gate chain is read once and not fetched.  Runs after fuse_pools and
    fuse_hard_activations and before fuse_conv, which would otherwise take the
    FCs and keep only bf16 weights."""
    _fuse_squeeze_excite(g, order, fed, fetch_refs, device, opts, "_HardSigmoid", ("Relu",), "_SqueezeExcite")


def fuse_squeeze_excite_sigmoid(g, order, fed, fetch_refs, device, opts):
    """fuse_squeeze_excite's pattern with a plain ``Sigmoid`` gate and a none /
    ``Relu`` / ``_Swish`` inner activation -> ``_SqueezeExciteSigmoid(x)``
    (EfficientNet), never ``_SqueezeExcite``.  Runs after fuse_swish, next to
    fuse_squeeze_excite."""
    _fuse_squeeze_excite(g, order, fed, fetch_refs, device, opts, "Sigmoid", ("Relu", "_Swish"),
                         "_SqueezeExciteSigmoid")


def _fuse_squeeze_excite(g, order, fed, fetch_refs, device, opts, gate_op, act1_ops, out_op):
    """The squeeze-excite pattern gated by ``gate_op`` with an inner activation
    of ``act1_ops`` (or none) -> ``out_op``."""
    c = _Ctx(g, order, fed, fetch_refs, device, opts)

    def up(ref, reader, ops):
        """The node behind ``ref`` if it is one of ``ops`` (output 0) read by ``reader`` alone."""
        n = g.nodes.get(ref[0])
        if n is None or ref[1] != 0 or n.op not in ops or c.only_consumer(n.name) is not reader:
            return None
        return n

    def fc(ref, reader):
        """([BiasAdd ->] Conv2D chain nodes reader-side first, conv, w, bias) behind ``ref``."""
        nodes = []
        ba = up(ref, reader, ("BiasAdd",))
        bias = None
        if ba is not None:
            bias = _const(g, ba.inputs[1])
            if bias is None or bias.dim() != 1 or ba.sattr("data_format", "NHWC") != "NHWC":
                return None
            nodes.append(ba)
            ref, reader = ba.inputs[0], ba
        conv = up(ref, reader, ("Conv2D",))
        w = _fc_1x1(g, conv)
        if w is None or (bias is not None and bias.numel() != w.shape[1]):
            return None
        nodes.append(conv)
        return nodes, conv, w, bias if bias is not None else zeros(w.shape[1], w)

    for name in order:
        m = g.nodes.get(name)
        if m is None or m.op != "Mul" or len(m.inputs) != 2:
            continue
        for x_ref, g_ref in ((m.inputs[0], m.inputs[1]), (m.inputs[1], m.inputs[0])):
            hs = up(g_ref, m, (gate_op,))
            if hs is None or x_ref == g_ref or len(hs.inputs) != 1:
                continue
            f2 = fc(hs.inputs[0], hs)
            if f2 is None:
                continue
            nodes2, conv2, w2, b2 = f2
            act1, reader, ref = "none", conv2, conv2.inputs[0]
            chain = [hs] + nodes2
            relu = up(ref, conv2, act1_ops)
            if relu is not None:
                act1, reader, ref = _CLOSING_ACTS[relu.op], relu, relu.inputs[0]
                chain.append(relu)
            f1 = fc(ref, reader)
            if f1 is None:
                continue
            nodes1, conv1, w1, b1 = f1
            chain += nodes1
            ch, cr = w1.shape
            if tuple(w2.shape) != (cr, ch):
                continue
            reshape = None
            ref, reader = conv1.inputs[0], conv1
            rs = up(ref, conv1, ("Reshape",))
            if rs is not None:
                shp = _const(g, rs.inputs[1])
                if shp is None or [int(v) for v in shp.reshape(-1).tolist()] != [-1, 1, 1, ch]:
                    continue
                reshape = [-1, 1, 1, ch]
                chain.append(rs)
                ref, reader = rs.inputs[0], rs
            pool = up(ref, reader, ("_GlobalAvgPool",))
            if pool is None or pool.inputs[0] != x_ref:
                continue
            pimpl = pool.attrs["_impl"]
            if not isinstance(pimpl, GlobalAvgPool) or pimpl.keep == (reshape is not None):
                continue
            chain.append(pool)
            impl = SqueezeExcite(w1, b1, w2, b2, act1, hs.attr("scale", 1.0 / 6.0), pimpl.keep, pimpl.axes, reshape,
                                 device, c.use_hip, m.name,
                                 gate="sigmoid" if gate_op == "Sigmoid" else "hard_sigmoid")
            _finalize(g, chain[::-1] + [m], out_op, [x_ref], {"_impl": impl})
            c.refresh()
            break


def _feeds_head(c: _Ctx, name: str, depth: int = 0) -> bool:
    if name in c.fetch_nodes:
        return True
    if depth > 3:
        return False
    for cname, _p, _i in c.cons.get(name, []):
        cn = c.g.nodes[cname]
        if cn.op in ("Softmax", "ArgMax", "_SoftmaxArgMax", "LogSoftmax", "TopKV2", "Sigmoid"):
            return True
        if cn.op in ("Identity", "Squeeze", "Reshape") and _feeds_head(c, cname, depth + 1):
            return True
    return False


GELU_ACTS = ("gelu_tanh", "gelu_erf")


def fuse_matmul(g, order, fed, fetch_refs, device, opts):
    c = _Ctx(g, order, fed, fetch_refs, device, opts)
    for name in order:
        n = g.nodes.get(name)
        if n is None or n.op != "MatMul" or n.attr("transpose_a", False):
            continue
        w = _const(g, n.inputs[1])
        if w is None or w.dim() != 2:
            continue
        w = w.float()
        if n.attr("transpose_b", False):
            w = w.t()
        kdim, ndim = w.shape
        chain = [n]
        cur = n
        bias = None
        residual = None
        act = "none"
        nxt = c.only_consumer(cur.name)
        if nxt is not None and nxt.op in ("BiasAdd", "Add", "AddV2") and nxt.inputs[0] == (cur.name, 0):
            # by shape, not by size: [N], [1,N] or one element (an [N,1] constant adds a column)
            b = _channel_const(_const(g, nxt.inputs[1]), ndim, 1 if nxt.op == "BiasAdd" else 2)
            if b is not None:
                bias = b.expand(ndim).contiguous()
                chain.append(nxt)
                cur = nxt
                nxt = c.only_consumer(cur.name)
        gelu = match_gelu(g, c, cur.name)
        if gelu is not None:
            act, gnodes, out_node = gelu
            chain += gnodes + [out_node]
            cur = out_node
        elif nxt is not None and nxt.op in ("Relu", "Tanh"):
            act = nxt.op.lower()
            chain.append(nxt)
            cur = nxt
        elif nxt is not None and nxt.op in ("Add", "AddV2") and len(nxt.inputs) == 2:
            other = nxt.inputs[1] if nxt.inputs[0] == (cur.name, 0) else nxt.inputs[0]
            if other != (cur.name, 0) and _const(g, other) is None:
                residual = other
                chain.append(nxt)
                cur = nxt
        out_f32 = _feeds_head(c, cur.name)
        cons = c.cons.get(cur.name, [])
        pad_n = cur.name not in c.fetch_nodes and bool(cons) and \
            all(g.nodes[cn].op == "_SoftmaxArgMax" for cn, _p, _i in cons)
        impl = FusedMatMul(w, bias, act, out_f32, device, c.use_hip, cur.name, pad_n)
        _finalize(g, chain, "_FusedMatMul", [n.inputs[0]] + ([residual] if residual else []), {"_impl": impl})
        c.refresh()


def match_gelu(g: Graph, c: _Ctx, src: str):
    """Match GELU applied to ``src`` (exactly-once uses):
    erf form:  0.5 * x * (1 + erf(x / sqrt(2)))   (any association order)
    tanh form: 0.5 * x * (1 + tanh(sqrt(2/pi) * (x + 0.044715 * x^3)))
    Returns (act, interior nodes, output node) or None."""
    from .patterns import match_gelu_subgraph
    return match_gelu_subgraph(g, c, src)


def fuse_pools(g, order, fed, fetch_refs, device, opts):
    c = _Ctx(g, order, fed, fetch_refs, device, opts)
    for name in order:
        n = g.nodes.get(name)
        if n is None:
            continue
        if n.op == "Mean":
            ax = _const(g, n.inputs[1])
            axes = None if ax is None else [int(a) for a in ax.reshape(-1).tolist()]
            if axes is not None and sorted(axes) in ([1, 2], [-3, -2]):
                # (H and W of an NHWC tensor if its rank is 4: the op checks, and keeps the axes for any other rank)
                n.op = "_GlobalAvgPool"
                n.attrs = {"_impl": GlobalAvgPool(bool(n.attr("keep_dims", False)), c.use_hip, axes)}
                n.inputs = [n.inputs[0]]
        elif n.op == "MaxPool" and n.sattr("data_format", "NHWC") == "NHWC":
            k, s = n.attr("ksize"), n.attr("strides")
            padding, pads = n.sattr("padding", "VALID"), (0, 0, 0, 0)
            if not (k[0] == k[3] == s[0] == s[3] == 1) or padding not in ("SAME", "VALID", "EXPLICIT"):
                continue
            if padding == "EXPLICIT":
                ep = list(n.attr("explicit_paddings", []) or [])
                if len(ep) != 8 or ep[0] or ep[1] or ep[6] or ep[7] or min(ep) < 0:
                    continue
                pads = (ep[2], ep[3], ep[4], ep[5])
                if max(pads[0], pads[1]) >= k[1] or max(pads[2], pads[3]) >= k[2]:
                    continue          # a window could lie wholly in the padding
            n.op = "_MaxPool"
            n.attrs = {"_impl": MaxPool((k[1], k[2]), (s[1], s[2]), padding, c.use_hip, pads)}


def fuse_softmax_argmax(g, order, fed, fetch_refs, device, opts):
    c = _Ctx(g, order, fed, fetch_refs, device, opts)
    by_input: Dict[tuple, Dict[str, Node]] = {}
    for name in order:
        n = g.nodes.get(name)
        if n is None or not n.inputs:
            continue
        if n.op == "Softmax":
            by_input.setdefault(n.inputs[0], {})["sm"] = n
        elif n.op == "ArgMax":
            ax = _const(g, n.inputs[1])
            if ax is not None and ax.numel() == 1 and int(ax.reshape(-1)[0]) in (1, -1):
                by_input.setdefault(n.inputs[0], {})["am"] = n
    for src, d in by_input.items():
        if "sm" in d and "am" in d:
            sm, am = d["sm"], d["am"]
            cdt = O.DT_TO_TORCH.get(am.attrs.get("output_type", T.DT_INT64), torch.int64)
            sm.op = "_SoftmaxArgMax"
            sm.attrs = {"_impl": SoftmaxArgMax(c.use_hip, cdt, int(_const(g, am.inputs[1]).reshape(-1)[0]))}
            am.op = "Identity"
            am.inputs = [(sm.name, 1)]
            am.attrs = {}


def _is_1x1(impl) -> bool:
    """A 1x1 conv without padding (SAME never pads a 1x1 filter)."""
    return isinstance(impl, FusedConv) and impl.kh == impl.kw == 1 and impl.use_hip and not impl.c4 and \
        (impl.padding != "EXPLICIT" or not any(impl.pads))


def fuse_dual_conv(g, order, fed, fetch_refs, device, opts):
    """Merge ``_FusedConv2D(a, residual=_FusedConv2D(b))`` where both are 1x1
    convs, the residual producer has no activation and no other consumer, and
    one of them has stride 1, into ``_FusedDualConv(h=stride-1 input, x=other
    input)`` (GPU only; both channel counts multiples of 64)."""
    c = _Ctx(g, order, fed, fetch_refs, device, opts)
    if not c.use_hip:
        return
    for name in order:
        n = g.nodes.get(name)
        if n is None or n.op != "_FusedConv2D" or len(n.inputs) != 2:
            continue
        a = n.attrs["_impl"]
        r = g.nodes.get(n.inputs[1][0])
        if r is None or r.op != "_FusedConv2D" or len(r.inputs) != 1 or n.inputs[1][1] != 0:
            continue
        b = r.attrs["_impl"]
        if not (_is_1x1(a) and _is_1x1(b)) or b.act != "none" or c.only_consumer(r.name) is not n:
            continue
        if a.act in IGEMM_ONLY_ACTS:
            continue                  # the dual conv is cgemm-only, and cgemm has no relu6 / hard_swish
        if a.cin % 64 or b.cin % 64 or a.cout != b.cout or a.cout % 8:
            continue
        # the stride-1 conv's input is the dense source (its rows are the output pixels)
        if a.sh == a.sw == 1:
            conv_h, h_ref, conv_x, x_ref = a, n.inputs[0], b, r.inputs[0]
        elif b.sh == b.sw == 1:
            conv_h, h_ref, conv_x, x_ref = b, r.inputs[0], a, n.inputs[0]
        else:
            continue
        impl = FusedDualConv(conv_h, conv_x, a.act, device, c.use_hip, n.name)
        n.op = "_FusedDualConv"
        n.inputs = [h_ref, x_ref]
        n.ctrl = _merge_ctrl([r, n])
        n.attrs = {"_impl": impl}
        del g.nodes[r.name]
        c.refresh()


def fuse_post_activation(g, order, fed, fetch_refs, device, opts):
    """ResNet v2 pre-activation: ``P -> FusedBatchNorm -> [Relu]`` where P is a
    fused conv / dual conv / max-pool becomes a second output of P written by
    the same kernel's epilogue: P then yields ``[sum, relu(bn(sum))]`` when the
    raw sum has other consumers (the next block's identity shortcut), or just
    ``[relu(bn(sum))]`` when it does not (a projecting next block; the final
    post-norm before the global pool).  SURVEY.md §2.7 K1's dual-output
    epilogue; the model is the reference's ``resnet_v2_fp32_savedmodel_NHWC``
    (``serving/fetch.sh:7``)."""
    c = _Ctx(g, order, fed, fetch_refs, device, opts)
    for name in order:
        p = g.nodes.get(name)
        if p is None or p.op not in ("_FusedConv2D", "_FusedDualConv", "_MaxPool"):
            continue
        impl = p.attrs["_impl"]
        if impl.post is not None or not impl.post_ok() or name in c.fetch_nodes:
            continue
        cons = c.cons.get(name, [])
        if any(i != 0 for _c, _p, i in cons):
            continue
        bns = [g.nodes[cn] for cn, _pos, _i in cons
               if g.nodes[cn].op.startswith("FusedBatchNorm") and g.nodes[cn].inputs[0] == (name, 0)]
        if len(bns) != 1:
            continue
        bn = bns[0]
        aff = _bn_affine(g, c, bn)
        if aff is None or aff[0].numel() != getattr(impl, "cout", aff[0].numel()):
            continue
        out_node, act = bn, "none"
        relu = c.only_consumer(bn.name)
        if relu is not None and relu.op == "Relu" and relu.name not in c.fetch_nodes:
            out_node, act = relu, "relu"
        elif bn.name in c.fetch_nodes:
            continue
        others = [cn for cn, _pos, _i in cons if cn != bn.name]
        if isinstance(impl, MaxPool) and others:
            continue                  # the pooling kernel writes one output
        mode = "dual" if others else "only"
        if isinstance(impl, MaxPool):
            impl.set_post(aff[0], aff[1], act, mode, device=c.device)
        else:
            impl.set_post(aff[0], aff[1], act, mode)
        new_ref = (name, 1 if mode == "dual" else 0)
        for cn, pos, _i in c.cons.get(out_node.name, []):
            g.nodes[cn].inputs[pos] = new_ref
        p.ctrl = _merge_ctrl([p, bn] + ([out_node] if out_node is not bn else []))
        del g.nodes[bn.name]
        if out_node is not bn:
            del g.nodes[out_node.name]
        c.refresh()


def _chainable_1x1(impl) -> bool:
    return (isinstance(impl, FusedConv) and impl.kh == 1 and impl.kw == 1 and impl.sh == 1 and impl.sw == 1 and
            not impl.c4 and impl.post is None and impl.act in ("relu", "none") and
            (impl.padding != "EXPLICIT" or not any(impl.pads)))


def fuse_conv_chain(g, order, fed, fetch_refs, device, opts):
    """``_FusedConv2D`` A (1x1 expand, optional residual) whose output feeds a
    ``_FusedConv2D`` B (1x1 reduce, no residual) -> ``_ChainConv`` with outputs
    ``[A, B]`` when (A.cin, A.cout, B.cout) is a kernel shape; A's other
    consumers (the next shortcut) keep reading output 0.  A may also be a
    stride-1 ``_FusedDualConv`` without a post output (inputs ``[h, x]``,
    shape (c1 + c2, cout, B.cout) in CHAIN_SHAPES_DUAL).  GPU programs only
    (``TFSERVE_CONV_CHAIN=0`` disables it, ``force`` applies it on CPU too:
    the op then runs both reference convs)."""
    import os
    mode = os.environ.get("TFSERVE_CONV_CHAIN", "1")
    shapes = CHAIN_SHAPES_STAGE1 if os.environ.get("TFSERVE_CONV_CHAIN_SHAPES") == "stage1" else CHAIN_SHAPES_ALL
    c = _Ctx(g, order, fed, fetch_refs, device, opts)
    if mode == "0" or (not c.use_hip and mode != "force"):
        return
    for name in order:
        p = g.nodes.get(name)
        if p is None or p.op not in ("_FusedConv2D", "_FusedDualConv") or name in c.fetch_nodes:
            continue
        a = p.attrs["_impl"]
        dual = p.op == "_FusedDualConv"
        if dual:
            if not (a.use_hip and a.sh == a.sw == 1 and a.post is None and a.act in ("relu", "none")):
                continue
        elif not _chainable_1x1(a):
            continue
        cons = c.cons.get(name, [])
        if any(i != 0 for _c, _p, i in cons):
            continue
        bs = [g.nodes[cn] for cn, pos, _i in cons
              if pos == 0 and g.nodes[cn].op == "_FusedConv2D" and len(g.nodes[cn].inputs) == 1 and
              cn not in c.fetch_nodes and _chainable_1x1(g.nodes[cn].attrs["_impl"])]
        if len(bs) != 1:
            continue
        bnode = bs[0]
        b = bnode.attrs["_impl"]
        shape = (a.c1 + a.c2 if dual else a.cin, a.cout, b.cout)
        if b.cin != a.cout or shape not in (CHAIN_SHAPES_DUAL if dual else shapes):
            continue
        chain = ChainConv(a, b)
        p.op = "_ChainConv"
        p.attrs = {"_impl": chain}
        for cn, pos, _i in c.cons.get(bnode.name, []):
            g.nodes[cn].inputs[pos] = (name, 1)
        p.ctrl = _merge_ctrl([p, bnode])
        del g.nodes[bnode.name]
        c.refresh()


def default_passes(options=None):
    from .patterns import bert_passes, dlrm_passes, late_passes
    return [fuse_pools, fuse_softmax_argmax, fuse_hard_activations, fuse_swish, fuse_squeeze_excite,
            fuse_squeeze_excite_sigmoid] + bert_passes() + dlrm_passes() + \
        [fuse_grouped_conv, fuse_conv, fuse_patch_tokens, fuse_depthwise, fuse_depthwise_layernorm,
         fuse_dual_conv, fuse_post_activation, fuse_stem_pool, fuse_matmul,
         fuse_classifier_head, fuse_dense_softmax, fuse_conv_chain] + late_passes() + \
        [fuse_matmul_layernorm, defer_layernorm, release_weight_sources]
