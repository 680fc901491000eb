"""Subgraph pattern matchers for encoder (BERT-style) graphs.

* decomposed LayerNorm (``tf.contrib.layers.layer_norm`` / BERT ``modeling.py``)::

      mean = Mean(x, -1, keep);  var = Mean(SquaredDifference(x, StopGradient(mean)), -1, keep)
      M = Mul(Rsqrt(AddV2(var, eps)), gamma)
      y = AddV2(Mul(x, M), Sub(beta, Mul(mean, M)))          => _LayerNorm(x)

* GELU, tanh form (BERT) and erf form (Keras/TF2)    => activation of _FusedMatMul
* self-attention core::

      q|k|v = Transpose(Reshape(BiasAdd(MatMul(x, Wq|k|v)), [-1,S,H,D]), [0,2,1,3])
      p = Softmax(AddV2(Mul(BatchMatMul(q, k, adj_y), scale), mask_adder))
      y = Reshape(Transpose(BatchMatMul(p, v), [0,2,1,3]), [-1, H*D])
        => _FusedQKV(x)  (one GEMM, concatenated weights)  ->  _Attention(qkv, mask_adder)

* Swin's windowed attention (``fuse_window_attention``) and the roll / partition /
  reverse layout around it (``fold_window_layout``)
        => _FusedQKV(x)  ->  _WindowAttention(qkv; bias, mask, grid)

Matching is strict: every interior node must be consumed only inside the
pattern; anything else is left to the reference ops.
"""
from __future__ import annotations

import math
import os
from typing import Dict, List, Optional, Sequence, Set, Tuple

import torch
import torch.nn.functional as F

from . import ops as O
from .placement import to_device
from .ir import Graph, Node

BF16 = torch.bfloat16


# ------------------------------------------------------------------ helpers
def _node(g: Graph, ref) -> Optional[Node]:
    return g.nodes.get(ref[0]) if ref[1] == 0 else None


def _const_t(g: Graph, ref) -> Optional[torch.Tensor]:
    n = g.nodes.get(ref[0])
    if n is None or n.op != "Const" or n.value is None:
        return None
    v = n.value[ref[1]]
    return v if isinstance(v, torch.Tensor) else None


def _scalar(g: Graph, ref) -> Optional[float]:
    v = _const_t(g, ref)
    if v is None or v.numel() != 1:
        return None
    return float(v.reshape(-1)[0])


def _other(n: Node, ref) -> Optional[tuple]:
    if len(n.inputs) != 2:
        return None
    if n.inputs[0] == ref:
        return n.inputs[1]
    if n.inputs[1] == ref:
        return n.inputs[0]
    return None


def _close(a: Optional[float], b: float, tol: float = 1e-4) -> bool:
    return a is not None and abs(a - b) <= tol * max(1.0, abs(b))


def _interior_ok(c, interior: Sequence[Node], out: Node) -> bool:
    names = {n.name for n in interior} | {out.name}
    for n in interior:
        if n.name in c.fetch_nodes:
            return False
        for cname, _p, _i in c.cons.get(n.name, []):
            if cname not in names:
                return False
    return True


def _consumers(c, name: str) -> List[Node]:
    return [c.g.nodes[cn] for cn, _p, _i in c.cons.get(name, [])]


def _remove(g: Graph, nodes: Sequence[Node]):
    for n in nodes:
        g.nodes.pop(n.name, None)


def _axes_last(g, ref, rank_hint=None) -> bool:
    v = _const_t(g, ref)
    if v is None or v.numel() != 1:
        return False
    a = int(v.reshape(-1)[0])
    return a == -1 or (rank_hint is not None and a == rank_hint - 1)


def _last_axis_const(v: torch.Tensor) -> Optional[torch.Tensor]:
    """``v`` flattened when it varies along its last axis only (shape, leading
    1s dropped, is ``(cols,)``, or it has one element), else None."""
    if v.numel() == 1:
        return v.reshape(1)
    shape = list(v.shape)
    while shape and shape[0] == 1:
        shape.pop(0)
    return v.reshape(-1) if len(shape) == 1 else None


# ------------------------------------------------------------------ fused impls
class LayerNormOp:
    def __init__(self, gamma, beta, eps, device, use_hip):
        self.eps = float(eps)
        self.use_hip = use_hip
        # [cols] vectors, or one element each (a scalar gamma / beta: expanded
        # to the row length, which only the call knows)
        self.g = to_device(gamma.float().reshape(-1), device)
        self.b = to_device(beta.float().reshape(-1), device)

        self._rows = None             # (cols, gamma [cols], beta [cols]) of a scalar gamma / beta, cached

    def params(self, cols: int):
        """(gamma, beta) as [cols] vectors; the op's own weights stay as they were bound."""
        if self.g.numel() == self.b.numel() and self.g.numel() != 1:
            return self.g, self.b
        if self._rows is None or self._rows[0] != cols:
            g = self.g.expand(cols).contiguous() if self.g.numel() == 1 else self.g
            b = self.b.expand(cols).contiguous() if self.b.numel() == 1 else self.b
            self._rows = (cols, g, b)
        return self._rows[1], self._rows[2]

    def __call__(self, ctx, node, ins):
        x = O.to_torch(ins[0])
        g, b = self.params(x.shape[-1])
        if self.use_hip and x.is_cuda and x.shape[-1] % 8 == 0 and x.shape[-1] == g.numel():
            from ..ops import hip
            from .fused import _to_bf16
            return [hip().layernorm(_to_bf16(x).contiguous(), None, g, b, self.eps)]
        y = F.layer_norm(x.float(), (x.shape[-1],), g.to(x.device), b.to(x.device), self.eps)
        return [y if not x.is_cuda else y.to(x.dtype)]


MAX_ATTENTION_SEQ = 4096      # kernels/launch.h kMaxAttentionSeq


class AttentionOp:
    def __init__(self, heads: int, head_dim: int, seq: int, scale: float, use_hip: bool):
        self.h, self.d, self.s, self.scale, self.use_hip = heads, head_dim, seq, scale, use_hip
        self.form = None              # None: ops.tuned_choice picks among attention_forms(S); 0 / 1 forced

    def __call__(self, ctx, node, ins):
        qkv = O.to_torch(ins[0])
        adder = O.to_torch(ins[1]) if len(ins) > 1 else None
        S, H, D = self.s, self.h, self.d
        B = qkv.numel() // (S * 3 * H * D)
        # the kernel's adder is [B|1, 1, S|1, S]: one for all heads.  Any other adder that broadcasts
        # against the [B, H, S, S] scores (a per-head [1, H, S, S] bias) takes the torch path below
        kernel_adder = adder is None or (adder.dim() == 4 and adder.shape[1] == 1 and adder.shape[-1] == S and
                                         adder.shape[0] in (1, B) and adder.shape[2] in (1, S))
        if self.use_hip and qkv.is_cuda and D == 64 and 1 <= S <= MAX_ATTENTION_SEQ and kernel_adder:
            from ..ops import hip
            from .fused import _to_bf16
            q3 = _to_bf16(qkv).reshape(B, S, 3 * H * D).contiguous()
            mask = None
            bstride = qstride = 0
            if adder is not None:
                mask = adder.float().contiguous().to(qkv.device)
                bstride = S * adder.shape[2] if adder.shape[0] == B and B > 1 else 0
                qstride = S if adder.shape[2] == S else 0
            kernels = hip()
            forms = [int(f) for f in kernels.attention_forms(S)]
            if len(forms) == 1:
                y = kernels.attention(q3, mask, H, self.scale, None, bstride, qstride)
                return [y.reshape(B * S, H * D)]
            # a length with two kernels (kernels/attention.hip: the KV-block loop, form 0, or the
            # register kernel padded to 32 keys, form 1): timed per shape under a key of its own
            out = torch.empty((B, S, H * D), device=q3.device, dtype=BF16)

            def run(form):
                return kernels.attention(q3, mask, H, self.scale, out, bstride, qstride, form)
            layout = "none" if mask is None else ("query" if qstride else "key")
            pick = self.form
            if pick is None:
                from ..ops import tuned_choice
                pick = tuned_choice(("attn", B, S, H, layout), {f: (lambda f=f: run(f)) for f in forms}, default=0)
            return [run(pick).reshape(B * S, H * D)]
        q, k, v = qkv.float().reshape(B, S, 3, H, D).permute(2, 0, 3, 1, 4)
        sc = q @ k.transpose(-1, -2) * self.scale
        if adder is not None:
            sc = sc + adder.float().to(sc.device)
        y = (torch.softmax(sc, -1) @ v).permute(0, 2, 1, 3).reshape(B * S, H * D)
        return [y if not qkv.is_cuda else y.to(qkv.dtype)]


# ------------------------------------------------------------------ GELU
def match_gelu_subgraph(g: Graph, c, src: str):
    x = (src, 0)
    cons = _consumers(c, src)
    if src in c.fetch_nodes:
        return None
    # tanh form
    pows = [n for n in cons if n.op == "Pow" and n.inputs[0] == x and _close(_scalar(g, n.inputs[1]), 3.0)]
    if pows:
        pw = pows[0]
        chain = [pw]
        nx = _consumers(c, pw.name)
        if len(nx) != 1 or nx[0].op != "Mul" or not _close(_scalar(g, _other(nx[0], (pw.name, 0))), 0.044715):
            return None
        m = nx[0]
        chain.append(m)
        nx = _consumers(c, m.name)
        if len(nx) != 1 or nx[0].op not in ("Add", "AddV2") or _other(nx[0], (m.name, 0)) != x:
            return None
        a = nx[0]
        chain.append(a)
        nx = _consumers(c, a.name)
        if len(nx) != 1 or nx[0].op != "Mul" or not _close(_scalar(g, _other(nx[0], (a.name, 0))),
                                                          math.sqrt(2 / math.pi)):
            return None
        m1 = nx[0]
        chain.append(m1)
        nx = _consumers(c, m1.name)
        if len(nx) != 1 or nx[0].op != "Tanh":
            return None
        t = nx[0]
        chain.append(t)
        tail = _gelu_tail(g, c, t, x, chain)
        if tail is None:
            return None
        return ("gelu_tanh",) + tail
    # erf form: Erf(x * 1/sqrt2) or Erf(x / sqrt2)
    for n in cons:
        if n.op == "Mul" and _close(_scalar(g, _other(n, x) or ("", 0)), 1 / math.sqrt(2)) or \
                n.op == "RealDiv" and n.inputs[0] == x and _close(_scalar(g, n.inputs[1]), math.sqrt(2)):
            nx = _consumers(c, n.name)
            if len(nx) == 1 and nx[0].op == "Erf":
                tail = _gelu_tail(g, c, nx[0], x, [n, nx[0]])
                if tail is not None:
                    return ("gelu_erf",) + tail
    return None


def _gelu_tail(g, c, t: Node, x, chain: List[Node]):
    """... t -> AddV2(1, t) -> [Mul(0.5, .) -> Mul(x, .)] | [Mul(., Mul(x, 0.5))]"""
    nx = _consumers(c, t.name)
    if len(nx) != 1 or nx[0].op not in ("Add", "AddV2") or not _close(_scalar(g, _other(nx[0], (t.name, 0))), 1.0):
        return None
    a1 = nx[0]
    chain = chain + [a1]
    nx = _consumers(c, a1.name)
    if len(nx) != 1 or nx[0].op != "Mul":
        return None
    m2 = nx[0]
    other = _other(m2, (a1.name, 0))
    if _close(_scalar(g, other), 0.5):            # 0.5 * (1 + t) then * x
        chain.append(m2)
        nx = _consumers(c, m2.name)
        if len(nx) != 1 or nx[0].op != "Mul" or _other(nx[0], (m2.name, 0)) != x:
            return None
        out = nx[0]
    elif other == x:                              # x * (1 + t) then * 0.5
        chain.append(m2)
        nx = _consumers(c, m2.name)
        if len(nx) != 1 or nx[0].op != "Mul" or not _close(_scalar(g, _other(nx[0], (m2.name, 0))), 0.5):
            return None
        out = nx[0]
    else:                                         # (x * 0.5) * (1 + t)
        h = _node(g, other) if other else None
        if h is None or h.op != "Mul" or _other(h, x) is None or not _close(_scalar(g, _other(h, x)), 0.5):
            return None
        chain = chain + [h]
        out = m2
    if not _interior_ok(c, chain, out):
        return None
    # every consumer of x must be inside the pattern (x is the GEMM output being fused)
    names = {n.name for n in chain} | {out.name}
    if any(n.name not in names for n in _consumers(c, x[0])):
        return None
    return chain, out


# ------------------------------------------------------------------ LayerNorm
def fuse_layernorm(g, order, fed, fetch_refs, device, opts):
    from .fused import _Ctx
    c = _Ctx(g, order, fed, fetch_refs, device, opts)
    for name in order:
        n = g.nodes.get(name)
        if n is None or n.op not in ("Add", "AddV2") or len(n.inputs) != 2:
            continue
        m = _match_ln(g, c, n)
        if m is None:
            continue
        x_ref, gamma, beta, eps, interior = m
        _remove(g, interior)
        n.op = "_LayerNorm"
        n.inputs = [x_ref]
        n.ctrl = []
        n.attrs = {"_impl": LayerNormOp(gamma, beta, eps, device, c.use_hip)}
        c.refresh()


def _match_ln(g, c, out: Node):
    for ia, ib in ((0, 1), (1, 0)):
        mul1, sub = _node(g, out.inputs[ia]), _node(g, out.inputs[ib])
        if mul1 is None or sub is None or mul1.op != "Mul" or sub.op != "Sub":
            continue
        beta = _const_t(g, sub.inputs[0])
        mul2 = _node(g, sub.inputs[1])
        if beta is None or mul2 is None or mul2.op != "Mul":
            continue
        for jx in (0, 1):
            x_ref = mul1.inputs[jx]
            M = _node(g, mul1.inputs[1 - jx])
            if M is None or M.op != "Mul":
                continue
            mean_ref = _other(mul2, (M.name, 0))
            mean = _node(g, mean_ref) if mean_ref else None
            if mean is None or mean.op != "Mean" or mean.inputs[0] != x_ref or not _axes_last(g, mean.inputs[1]):
                continue
            rs = gamma = None
            for k in (0, 1):
                a, b = _node(g, M.inputs[k]), _const_t(g, M.inputs[1 - k])
                if a is not None and a.op == "Rsqrt" and b is not None:
                    rs, gamma = a, b
            if rs is None:
                continue
            add = _node(g, rs.inputs[0])
            if add is None or add.op not in ("Add", "AddV2"):
                continue
            var = eps = None
            for k in (0, 1):
                a, e = _node(g, add.inputs[k]), _scalar(g, add.inputs[1 - k])
                if a is not None and a.op == "Mean" and e is not None:
                    var, eps = a, e
            if var is None or not _axes_last(g, var.inputs[1]):
                continue
            sqd = _node(g, var.inputs[0])
            if sqd is None or sqd.op != "SquaredDifference" or sqd.inputs[0] != x_ref:
                continue
            mref = sqd.inputs[1]
            sg = _node(g, mref)
            interior = [mul1, sub, mul2, M, mean, rs, add, var, sqd]
            if sg is not None and sg.op in ("StopGradient", "Identity"):
                if sg.inputs[0] != (mean.name, 0):
                    continue
                interior.append(sg)
            elif mref != (mean.name, 0):
                continue
            if not _interior_ok(c, interior, out):
                continue
            # the statistics broadcast against x only with keep_dims; gamma and beta must scale along the
            # last axis alone: a vector, [1, ..., cols], or one element (a [S, 1] constant is per row)
            if not (mean.attr("keep_dims", False) and var.attr("keep_dims", False)):
                continue
            gv, bv = _last_axis_const(gamma), _last_axis_const(beta)
            if gv is None or bv is None or (gv.numel() != bv.numel() and 1 not in (gv.numel(), bv.numel())):
                continue
            return x_ref, gv, bv, eps, interior
    return None


# ------------------------------------------------------------------ attention
def _dense_src(g, c, ref):
    """ref = BiasAdd(MatMul(x, W), b) (or MatMul alone) -> (x, W[K,N], b, nodes)."""
    n = _node(g, ref)
    nodes = []
    bias = None
    if n is not None and n.op in ("BiasAdd", "Add", "AddV2"):
        b = _const_t(g, n.inputs[1])
        # by shape, not by size: [N], [1, N] or one element (an [M, 1] constant adds a column)
        bias = None if b is None or b.dim() > 2 else _last_axis_const(b.float())
        if bias is None:
            return None
        nodes.append(n)
        n = _node(g, n.inputs[0])
    if n is None or n.op != "MatMul" or n.attr("transpose_a", False):
        return None
    w = _const_t(g, n.inputs[1])
    if w is None:
        return None
    w = w.float()
    if n.attr("transpose_b", False):
        w = w.t()
    nodes.append(n)
    if bias is None:
        bias = torch.zeros(w.shape[1], device=w.device)
    elif bias.numel() == 1:
        bias = bias.expand(w.shape[1]).contiguous()
    elif bias.numel() != w.shape[1]:
        return None
    return n.inputs[0], w, bias, nodes


def _heads_of(g, c, ref, S_expected=None):
    """ref = Transpose(Reshape(dense, [-1,S,H,D]), [0,2,1,3]) -> (dense ref, S, H, D, nodes)."""
    t = _node(g, ref)
    if t is None or t.op != "Transpose":
        return None
    perm = _const_t(g, t.inputs[1])
    if perm is None or perm.reshape(-1).tolist() != [0, 2, 1, 3]:
        return None
    r = _node(g, t.inputs[0])
    if r is None or r.op != "Reshape":
        return None
    shp = _const_t(g, r.inputs[1])
    if shp is None or shp.numel() != 4:
        return None
    _b, S, H, D = [int(v) for v in shp.reshape(-1).tolist()]
    if S <= 0 or H <= 0 or D <= 0:
        return None
    return r.inputs[0], S, H, D, [t, r]


def fuse_attention(g, order, fed, fetch_refs, device, opts):
    from .fused import FusedMatMul, _Ctx
    c = _Ctx(g, order, fed, fetch_refs, device, opts)
    for name in list(order):
        out = g.nodes.get(name)
        if out is None or out.op != "Reshape":
            continue
        t2 = _node(g, out.inputs[0])
        if t2 is None or t2.op != "Transpose":
            continue
        perm = _const_t(g, t2.inputs[1])
        if perm is None or perm.reshape(-1).tolist() != [0, 2, 1, 3]:
            continue
        pv = _node(g, t2.inputs[0])
        if pv is None or pv.op not in ("BatchMatMul", "BatchMatMulV2", "BatchMatMulV3") or \
                pv.attr("adj_x", False) or pv.attr("adj_y", False):
            continue
        sm = _node(g, pv.inputs[0])
        if sm is None or sm.op != "Softmax":
            continue
        cur = _node(g, sm.inputs[0])
        adder_ref = None
        scale = 1.0
        interior = [t2, pv, sm]
        if cur is not None and cur.op in ("Add", "AddV2"):
            # scores + adder (either order): scores side is the Mul/BatchMatMul
            a0, a1 = _node(g, cur.inputs[0]), _node(g, cur.inputs[1])
            if a0 is not None and a0.op in ("Mul", "RealDiv", "BatchMatMul", "BatchMatMulV2", "BatchMatMulV3"):
                adder_ref, cur2 = cur.inputs[1], a0
            else:
                adder_ref, cur2 = cur.inputs[0], a1
            interior.append(cur)
            cur = cur2
        if cur is not None and cur.op == "Mul":
            sv = None
            for k in (0, 1):
                s = _scalar(g, cur.inputs[k])
                if s is not None:
                    sv, nxt = s, _node(g, cur.inputs[1 - k])
            if sv is None:
                continue
            scale = sv
            interior.append(cur)
            cur = nxt
        elif cur is not None and cur.op == "RealDiv" and len(cur.inputs) == 2:
            # the TF ViT spelling: scores / sqrt(d).  Only a scalar divisor (by shape: a [S] constant
            # of equal entries is not one), never zero, and only on the right
            dv = _const_t(g, cur.inputs[1])
            if dv is None or dv.numel() != 1 or dv.dim() != 0 or not dv.is_floating_point() or float(dv) == 0.0:
                continue
            scale = 1.0 / float(dv)
            interior.append(cur)
            cur = _node(g, cur.inputs[0])
        qk = cur
        if qk is None or qk.op not in ("BatchMatMul", "BatchMatMulV2", "BatchMatMulV3") or \
                qk.attr("adj_x", False) or not qk.attr("adj_y", False):
            continue
        interior.append(qk)
        hq, hk, hv = _heads_of(g, c, qk.inputs[0]), _heads_of(g, c, qk.inputs[1]), _heads_of(g, c, pv.inputs[1])
        if hq is None or hk is None or hv is None:
            continue
        S, H, D = hq[1], hq[2], hq[3]
        if (hk[1], hk[2], hk[3]) != (S, H, D) or (hv[1], hv[2], hv[3]) != (S, H, D):
            continue
        fshape = _const_t(g, out.inputs[1])
        if fshape is None or fshape.numel() != 2 or fshape.reshape(-1).tolist()[-1] != H * D:
            continue                  # (the op returns [B * S, H * D])
        dq, dk, dv = _dense_src(g, c, hq[0]), _dense_src(g, c, hk[0]), _dense_src(g, c, hv[0])
        interior += hq[4] + hk[4] + hv[4]
        if dq and dk and dv and dq[0] == dk[0] == dv[0]:
            qkv_nodes = dq[3] + dk[3] + dv[3]
            if not _interior_ok(c, interior + qkv_nodes, out):
                continue
            w = torch.cat([dq[1], dk[1], dv[1]], dim=1)
            b = torch.cat([dq[2], dk[2], dv[2]])
            qkv_name = g.unique_name(out.name + "/fused_qkv")
            qkv = Node(name=qkv_name, op="_FusedQKV", inputs=[dq[0]],
                       attrs={"_impl": FusedMatMul(w, b, "none", False, device, c.use_hip, qkv_name)})
            g.add(qkv)
            _remove(g, interior + qkv_nodes)
            out.op = "_Attention"
            out.inputs = [(qkv_name, 0)] + ([adder_ref] if adder_ref is not None else [])
            out.ctrl = []
            out.attrs = {"_impl": AttentionOp(H, D, S, scale, c.use_hip)}
        else:
            # projections not fusable into one GEMM: keep them, concatenate outputs at run time
            continue
        c.refresh()


# ------------------------------------------------------------------ windowed attention (Swin)
WATTN_HEAD_DIM = 32           # kernels/launch.h kWattnHeadDim
WATTN_MAX_SEQ = 64            # kernels/launch.h kWattnMaxSeq
_BMM = ("BatchMatMul", "BatchMatMulV2", "BatchMatMulV3")


def window_partition(x: torch.Tensor, ws: int) -> torch.Tensor:
    """[B, Hf, Wf, C] -> [B * nW, ws * ws, C], windows row-major within an image."""
    B, Hf, Wf, C = x.shape
    x = x.reshape(B, Hf // ws, ws, Wf // ws, ws, C).permute(0, 1, 3, 2, 4, 5)
    return x.reshape(-1, ws * ws, C)


def window_reverse(x: torch.Tensor, ws: int, Hf: int, Wf: int) -> torch.Tensor:
    """The inverse of window_partition: [B * nW, ws * ws, C] -> [B, Hf, Wf, C]."""
    C = x.shape[-1]
    x = x.reshape(-1, Hf // ws, Wf // ws, ws, ws, C).permute(0, 1, 3, 2, 4, 5)
    return x.reshape(-1, Hf, Wf, C)


class WindowAttentionOp:
    """softmax(q k^T * scale + bias[h] (+ mask[w])) v within windows of ``s``
    tokens over a packed QKV buffer [R, 3 * H * D].  ``grid`` None: window bw
    owns rows [bw * s, (bw + 1) * s) and its mask window is bw % nW.  ``grid`` =
    (Hf, Wf, ws, shift), set by fold_window_layout: the rows are in image order
    and the op addresses the (shifted) windows itself, reading and writing in
    place.  The kernel (kernels/wattn.hip) runs on the device for D = 32 and
    s <= 64; the same mathematics with torch anywhere else, and always on the
    CPU.  ``TFSERVE_WATTN=0`` forces the torch path (A/B only)."""

    def __init__(self, heads: int, head_dim: int, seq: int, scale: float, bias: torch.Tensor,
                 mask: Optional[torch.Tensor], device, use_hip: bool):
        self.h, self.d, self.s, self.scale, self.use_hip = heads, head_dim, seq, float(scale), use_hip
        self.grid = None
        self.bias = to_device(bias.float().reshape(heads, seq, seq).contiguous(), device)
        self.mask = None if mask is None else to_device(mask.float().reshape(-1, seq, seq).contiguous(), device)
        self.nw = 0 if self.mask is None else int(self.mask.shape[0])

    def kernel_ok(self, qkv: torch.Tensor) -> bool:
        if not (self.use_hip and qkv.is_cuda and self.d == WATTN_HEAD_DIM and self.s <= WATTN_MAX_SEQ):
            return False
        if os.environ.get("TFSERVE_WATTN", "1") == "0":
            return False
        from ..ops import hip
        R = qkv.numel() // (3 * self.h * self.d)
        return bool(hip().window_attention_supported(R, self.s, self.h, self.d, self.nw,
                                                     None if self.grid is None else list(self.grid)))

    def _windows(self, qkv: torch.Tensor) -> torch.Tensor:
        """The attention of rows in window order, [Bw * s, 3 * H * D] -> [Bw * s, H * D], in fp32."""
        S, H, D = self.s, self.h, self.d
        Bw = qkv.shape[0] // S
        q, k, v = qkv.float().reshape(Bw, S, 3, H, D).permute(2, 0, 3, 1, 4)
        sc = q @ k.transpose(-1, -2) * self.scale + self.bias.to(qkv.device)[None]
        if self.mask is not None:
            if Bw % self.nw:
                raise O.OpError(f"{Bw} windows do not reshape to [-1, {self.nw}, {H}, {S}, {S}]")
            sc = (sc.reshape(-1, self.nw, H, S, S) + self.mask.to(qkv.device)[None, :, None]).reshape(Bw, H, S, S)
        return (torch.softmax(sc, -1) @ v).permute(0, 2, 1, 3).reshape(Bw * S, H * D)

    def __call__(self, ctx, node, ins):
        qkv = O.to_torch(ins[0])
        S, H, D = self.s, self.h, self.d
        W3 = 3 * H * D
        if qkv.numel() % W3:
            raise O.OpError(f"{node.name}: {list(qkv.shape)} is not [R, {W3}]")
        R = qkv.numel() // W3
        per = S if self.grid is None else self.grid[0] * self.grid[1]
        if R % per:
            raise O.OpError(f"{node.name}: {R} rows are not whole {'windows' if self.grid is None else 'maps'} of {per}")
        qkv = qkv.reshape(R, W3)
        if self.kernel_ok(qkv):
            from ..ops import hip
            from .fused import _to_bf16
            return [hip().window_attention(_to_bf16(qkv).contiguous(), self.bias, self.mask, H, self.scale, None,
                                           None if self.grid is None else list(self.grid))]
        if self.grid is None:
            y = self._windows(qkv)
        else:
            Hf, Wf, ws, sh = self.grid
            x = qkv.reshape(-1, Hf, Wf, W3)
            if sh:
                x = torch.roll(x, (-sh, -sh), (1, 2))
            y = window_reverse(self._windows(window_partition(x, ws).reshape(-1, W3)), ws, Hf, Wf)
            if sh:
                y = torch.roll(y, (sh, sh), (1, 2))
            y = y.reshape(R, H * D)
        return [y if not qkv.is_cuda else y.to(BF16)]


def _ints(g, ref) -> Optional[List[int]]:
    v = _const_t(g, ref)
    if v is None or v.is_floating_point():
        return None
    return [int(x) for x in v.reshape(-1).tolist()]


def _scale_of(g, n: Optional[Node]):
    """n = Mul(x, c) (either order) or RealDiv(x, c) with a scalar c under fuse_attention's rules
    -> (scale, x ref), else None."""
    if n is None or len(n.inputs) != 2:
        return None
    if n.op == "Mul":
        for k in (0, 1):
            s = _scalar(g, n.inputs[k])
            if s is not None:
                return s, n.inputs[1 - k]
    if n.op == "RealDiv":
        dv = _const_t(g, n.inputs[1])
        if dv is not None and dv.numel() == 1 and dv.dim() == 0 and dv.is_floating_point() and float(dv) != 0.0:
            return 1.0 / float(dv), n.inputs[0]
    return None


def _packed_qkv(g, q_ref, k_ref, v_ref):
    """q, k, v = Unpack(Transpose(Reshape(dense, [-1, S, 3, H, D]), [2, 0, 3, 1, 4])) -> (dense ref, S, H, D, nodes)."""
    un = g.nodes.get(q_ref[0])
    if un is None or un.op != "Unpack" or int(un.attr("axis", 0)) != 0:
        return None
    if (q_ref, k_ref, v_ref) != ((un.name, 0), (un.name, 1), (un.name, 2)):
        return None
    t = _node(g, un.inputs[0])
    if t is None or t.op != "Transpose" or _ints(g, t.inputs[1]) != [2, 0, 3, 1, 4]:
        return None
    r = _node(g, t.inputs[0])
    shp = _ints(g, r.inputs[1]) if r is not None and r.op == "Reshape" else None
    if shp is None or len(shp) != 5 or shp[0] != -1 or shp[2] != 3 or min(shp[1:]) <= 0:
        return None
    return r.inputs[0], shp[1], shp[3], shp[4], [un, t, r]


def fuse_window_attention(g, order, fed, fetch_refs, device, opts):
    """Swin's attention core -> _FusedQKV -> _WindowAttention (see the module
    docstring of kernels/wattn.hip for the arithmetic)::

        scores = BatchMatMul(q', k, adj_y)                  q' = q or Mul(q, c)
        scores = Mul(scores, c) | RealDiv(scores, c)        (at most one scale in all)
        biased = AddV2(scores, bias)                        bias a constant [1, H, S, S] | [H, S, S]
        masked = Reshape(AddV2(Reshape(biased, [-1, nW, H, S, S]), mask), [-1, H, S, S])     (optional)
                                                            mask a constant [1, nW, 1, S, S] | [nW, 1, S, S]
        y = Reshape(Transpose(BatchMatMul(Softmax(masked | biased), v), [0, 2, 1, 3]), [-1, H * D])

    q, k, v from one packed dense (``_packed_qkv``: its columns are already in
    the kernel's (3, H, D) order) or from three denses (``_heads_of``).  Only
    D = 32: any other head width is fuse_attention's.  S is not limited here:
    windows of more than 64 tokens (window 12) fuse too, and WindowAttentionOp then
    computes them with torch on the device, in fp32 -- the kernel holds 64 keys."""
    from .fused import FusedMatMul, _Ctx
    c = _Ctx(g, order, fed, fetch_refs, device, opts)
    for name in list(order):
        out = g.nodes.get(name)
        if out is None or out.op != "Reshape":
            continue
        t2 = _node(g, out.inputs[0])
        if t2 is None or t2.op != "Transpose" or _ints(g, t2.inputs[1]) != [0, 2, 1, 3]:
            continue
        pv = _node(g, t2.inputs[0])
        if pv is None or pv.op not in _BMM or pv.attr("adj_x", False) or pv.attr("adj_y", False):
            continue
        sm = _node(g, pv.inputs[0])
        if sm is None or sm.op != "Softmax":
            continue
        interior = [t2, pv, sm]
        cur = _node(g, sm.inputs[0])
        mask = None
        mshape = None
        if cur is not None and cur.op == "Reshape":
            # the shift mask: Reshape [-1, H, S, S] of AddV2(Reshape [-1, nW, H, S, S], mask)
            back = _ints(g, cur.inputs[1])
            add = _node(g, cur.inputs[0])
            if back is None or len(back) != 4 or add is None or add.op not in ("Add", "AddV2") or len(add.inputs) != 2:
                continue
            for k in (0, 1):
                r5, mv = _node(g, add.inputs[k]), _const_t(g, add.inputs[1 - k])
                if r5 is not None and r5.op == "Reshape" and mv is not None:
                    break
            else:
                continue
            mshape = _ints(g, r5.inputs[1])
            if mshape is None or len(mshape) != 5 or mshape[0] != -1 or back != [-1] + mshape[2:]:
                continue
            nW = mshape[1]
            if tuple(mv.shape) not in ((1, nW, 1, mshape[3], mshape[4]), (nW, 1, mshape[3], mshape[4])) or nW < 1:
                continue
            mask = mv
            interior += [cur, add, r5]
            cur = _node(g, r5.inputs[0])
        if cur is None or cur.op not in ("Add", "AddV2") or len(cur.inputs) != 2:
            continue
        for k in (0, 1):
            bias, sc = _const_t(g, cur.inputs[1 - k]), _node(g, cur.inputs[k])
            if bias is not None and sc is not None:
                break
        else:
            continue
        interior.append(cur)
        scale = None
        sv = _scale_of(g, sc) if sc.op in ("Mul", "RealDiv") else None
        if sv is not None:
            scale = sv[0]
            interior.append(sc)
            sc = _node(g, sv[1])
        qk = sc
        if qk is None or qk.op not in _BMM or qk.attr("adj_x", False) or not qk.attr("adj_y", False):
            continue
        interior.append(qk)
        q_ref, k_ref, v_ref = qk.inputs[0], qk.inputs[1], pv.inputs[1]
        qm = _node(g, q_ref)
        if scale is None and qm is not None and qm.op == "Mul":
            sv = _scale_of(g, qm)
            if sv is None:
                continue
            scale, q_ref = sv
            interior.append(qm)
        packed = _packed_qkv(g, q_ref, k_ref, v_ref)
        if packed is not None:
            dense_ref, S, H, D, nodes = packed
            interior += nodes
            ds = _dense_src(g, c, dense_ref)
            if ds is None or ds[1].shape[1] != 3 * H * D:
                continue
            x_ref, w, b, qkv_nodes = ds
        else:
            hq, hk, hv = _heads_of(g, c, q_ref), _heads_of(g, c, k_ref), _heads_of(g, c, v_ref)
            if hq is None or hk is None or hv is None or hq[1:4] != hk[1:4] or hq[1:4] != hv[1:4]:
                continue
            S, H, D = hq[1:4]
            interior += hq[4] + hk[4] + hv[4]
            dq, dk, dv = _dense_src(g, c, hq[0]), _dense_src(g, c, hk[0]), _dense_src(g, c, hv[0])
            if not (dq and dk and dv and dq[0] == dk[0] == dv[0]):
                continue
            if any(d[1].shape[1] != H * D for d in (dq, dk, dv)):
                continue
            x_ref = dq[0]
            w = torch.cat([dq[1], dk[1], dv[1]], dim=1)
            b = torch.cat([dq[2], dk[2], dv[2]])
            qkv_nodes = dq[3] + dk[3] + dv[3]
        if D != WATTN_HEAD_DIM:
            continue
        if tuple(bias.shape) not in ((1, H, S, S), (H, S, S)) or not bias.is_floating_point():
            continue                  # by shape: a [1, 1, S, S] adder is fuse_attention's
        if mask is not None and (mshape[2:] != [H, S, S] or not mask.is_floating_point()):
            continue
        if _ints(g, out.inputs[1]) != [-1, H * D]:
            continue                  # (the op returns [R, H * D])
        if not _interior_ok(c, interior + qkv_nodes, out):
            continue
        qkv_name = g.unique_name(out.name + "/fused_qkv")
        g.add(Node(name=qkv_name, op="_FusedQKV", inputs=[x_ref],
                   attrs={"_impl": FusedMatMul(w, b, "none", False, device, c.use_hip, qkv_name)}))
        _remove(g, interior + qkv_nodes)
        out.op = "_WindowAttention"
        out.inputs = [(qkv_name, 0)]
        out.ctrl = []
        out.attrs = {"_impl": WindowAttentionOp(H, D, S, 1.0 if scale is None else scale, bias, mask, device,
                                                c.use_hip)}
        c.refresh()


def _reshape_to(g, n: Optional[Node], want: Sequence[int]) -> bool:
    return n is not None and n.op == "Reshape" and _ints(g, n.inputs[1]) == list(want)


def _roll_of(g, n: Optional[Node]):
    """n = Roll(x, [a, b], [1, 2]) with constant operands -> (a, b), else None."""
    if n is None or n.op != "Roll" or len(n.inputs) != 3:
        return None
    shifts, axes = _ints(g, n.inputs[1]), _ints(g, n.inputs[2])
    if shifts is None or axes != [1, 2] or len(shifts) != 2:
        return None
    return shifts[0], shifts[1]


def _is_map(g, ref, Hf: int, Wf: int, C: int) -> bool:
    """Whether ``ref`` is provably [.., Hf, Wf, C]: a Reshape to the constant [-1, Hf, Wf, C], or a
    Placeholder declared with that static shape.  (The compiler infers no other shapes.)"""
    n = _node(g, ref)
    if _reshape_to(g, n, [-1, Hf, Wf, C]):
        return True
    if n is not None and n.op == "Placeholder":
        shape = n.attrs.get("shape")
        return isinstance(shape, tuple) and len(shape) == 4 and tuple(shape[1:]) == (Hf, Wf, C)
    return False


def _window_chain_up(g, qkv: Node, S: int, C: int, nw: int):
    """[Reshape [-1, C]] <- Reshape [-1, S, C] <- Transpose <- Reshape 6-D <- [Roll] <- x, walked up from the
    QKV GEMM -> (x ref, (Hf, Wf, ws, shift), (nwy, nwx), nodes), or None on a miss."""
    nodes = []
    up = _node(g, qkv.inputs[0])
    if _reshape_to(g, up, [-1, C]):
        nodes.append(up)
        up = _node(g, up.inputs[0])
    if not _reshape_to(g, up, [-1, S, C]):
        return None
    tp = _node(g, up.inputs[0])
    if tp is None or tp.op != "Transpose" or _ints(g, tp.inputs[1]) != [0, 1, 3, 2, 4, 5]:
        return None
    r6 = _node(g, tp.inputs[0])
    s6 = _ints(g, r6.inputs[1]) if r6 is not None and r6.op == "Reshape" else None
    if s6 is None or len(s6) != 6 or s6[0] != -1 or min(s6[1:]) <= 0 or s6[2] != s6[4] or s6[5] != C:
        return None
    nwy, ws, nwx = s6[1], s6[2], s6[3]
    Hf, Wf = nwy * ws, nwx * ws
    if ws * ws != S or (nw and nw != nwy * nwx):
        return None
    nodes += [up, tp, r6]
    x_ref, shift = r6.inputs[0], 0
    roll = _node(g, x_ref)
    if roll is not None and roll.op == "Roll":
        by = _roll_of(g, roll)
        if by is None or by[0] != by[1] or not -ws < by[0] < 0:
            return None
        # the Roll turns axes 1 and 2 of what it is given, the kernel an Hf x Wf map: they are the same
        # only if the rolled tensor is [.., Hf, Wf, C].  (Without a Roll the flattening is layout-neutral.)
        if not _is_map(g, roll.inputs[0], Hf, Wf, C):
            return None
        shift = -by[0]
        nodes.append(roll)
        x_ref = roll.inputs[0]
    return x_ref, (Hf, Wf, ws, shift), (nwy, nwx), nodes


def _window_chain_down(g, c, att: Node, C: int, grid, nwin):
    """dense -> Reshape [-1, ws, ws, C] -> Reshape 6-D -> Transpose -> Reshape [-1, Hf, Wf, C] -> [Roll], walked
    down from the attention -> (projection's last node, the chain's last node, nodes between), or None."""
    Hf, Wf, ws, shift = grid
    mm = c.only_consumer(att.name)
    if mm is None or mm.op != "MatMul" or mm.inputs[0] != (att.name, 0) or mm.attr("transpose_a", False):
        return None
    wv = _const_t(g, mm.inputs[1])
    if wv is None or wv.dim() != 2 or wv.shape[0 if mm.attr("transpose_b", False) else 1] != C:
        return None
    nodes, proj = [], mm
    nxt = c.only_consumer(mm.name)
    if nxt is not None and nxt.op in ("BiasAdd", "Add", "AddV2") and nxt.inputs[0] == (mm.name, 0):
        bv = _const_t(g, nxt.inputs[1])
        if bv is not None and bv.dim() <= 2 and _last_axis_const(bv) is not None:
            nodes.append(mm)
            proj = nxt
            nxt = c.only_consumer(proj.name)
    for want in ([-1, ws, ws, C], [-1, nwin[0], nwin[1], ws, ws, C]):
        if not _reshape_to(g, nxt, want):
            return None
        nodes.append(nxt)
        nxt = c.only_consumer(nxt.name)
    if nxt is None or nxt.op != "Transpose" or _ints(g, nxt.inputs[1]) != [0, 1, 3, 2, 4, 5]:
        return None
    nodes.append(nxt)
    last = c.only_consumer(nxt.name)
    if not _reshape_to(g, last, [-1, Hf, Wf, C]):
        return None
    if shift:
        nodes.append(last)
        last = c.only_consumer(last.name)
        if _roll_of(g, last) != (shift, shift):
            return None
    elif any(g.nodes[cn].op == "Roll" for cn, _p, _i in c.cons.get(last.name, [])):
        return None                   # a roll on the way out only: not this chain
    return proj, last, nodes


def fold_window_layout(g, order, fed, fetch_refs, device, opts):
    """Directly after fuse_window_attention: LayerNorm, the QKV GEMM and the
    output projection are per token, so they commute with the window
    permutation.  The chain::

        x [B, Hf, Wf, C] -> [Roll(-s, -s; axes 1, 2)]
          -> Reshape [-1, Hf/ws, ws, Wf/ws, ws, C] -> Transpose [0, 1, 3, 2, 4, 5] -> Reshape [-1, ws*ws, C]
          -> [Reshape [-1, C]] -> _FusedQKV -> _WindowAttention -> dense
          -> Reshape [-1, ws, ws, C]
          -> Reshape [-1, Hf/ws, Wf/ws, ws, ws, C] -> Transpose [0, 1, 3, 2, 4, 5] -> Reshape [-1, Hf, Wf, C]
          -> [Roll(+s, +s; axes 1, 2)]

    becomes Reshape(x, [-1, C]) -> _FusedQKV -> _WindowAttention(grid = (Hf, Wf,
    ws, s)) -> dense -> Reshape [-1, Hf, Wf, C]; a following Reshape [-1, C] of
    that reads the dense directly, so the block's residual add meets the GEMM.
    Every shape constant must agree, the rolls must be exact inverses with
    0 < s < ws (or both absent), a rolled x must be provably [.., Hf, Wf, C]
    (``_is_map``), and every interior node must have one reader and not be
    fetched; anything else keeps the op between its layout nodes.  The fold
    does not depend on the kernel: an op that takes its torch path (S > 64)
    rolls and partitions inside itself.  ``TFSERVE_WATTN_FOLD=0`` turns the
    pass off (A/B only)."""
    from .fused import _Ctx
    if os.environ.get("TFSERVE_WATTN_FOLD", "1") == "0":
        return
    c = _Ctx(g, order, fed, fetch_refs, device, opts)
    for name in list(order):
        att = g.nodes.get(name)
        if att is None or att.op != "_WindowAttention" or att.attrs["_impl"].grid is not None:
            continue
        impl = att.attrs["_impl"]
        C = impl.h * impl.d
        qkv = _node(g, att.inputs[0])
        if qkv is None or qkv.op != "_FusedQKV" or qkv.attrs["_impl"].k != C:
            continue
        up = _window_chain_up(g, qkv, impl.s, C, impl.nw)
        if up is None:
            continue
        x_ref, grid, nwin, before = up
        down = _window_chain_down(g, c, att, C, grid, nwin)
        if down is None:
            continue
        proj, last, after = down
        if not _interior_ok(c, [qkv, att, proj] + before + after, last):
            continue
        # ---- rewire
        flat_name = g.unique_name(att.name + "/rows")
        shape_name = g.unique_name(att.name + "/rows/shape")
        g.add(Node(name=shape_name, op="Const", inputs=[], attrs={}, value=[torch.tensor([-1, C], dtype=torch.int32)]))
        g.add(Node(name=flat_name, op="Reshape", inputs=[x_ref, (shape_name, 0)], attrs={}))
        qkv.inputs = [(flat_name, 0)]
        impl.grid = grid
        map_shape = g.unique_name(att.name + "/map/shape")
        g.add(Node(name=map_shape, op="Const", inputs=[], attrs={},
                   value=[torch.tensor([-1, grid[0], grid[1], C], dtype=torch.int32)]))
        mm = _node(g, proj.inputs[0]) if proj.op != "MatMul" else proj
        _remove(g, [n for n in before + after if n not in (mm, proj)])
        last.op = "Reshape"
        last.inputs = [(proj.name, 0), (map_shape, 0)]
        last.ctrl = []
        last.attrs = {}
        last.value = None
        c.refresh()
        # a Reshape [-1, C] of the map reads the projection's [R, C] rows as they are
        if last.name in c.fetch_nodes:
            continue
        for cn, _p, _i in list(c.cons.get(last.name, [])):
            rs = g.nodes[cn]
            if _reshape_to(g, rs, [-1, C]) and rs.inputs[0] == (last.name, 0) and rs.name not in c.fetch_nodes:
                for user in g.nodes.values():
                    user.inputs = [(proj.name, 0) if ref == (rs.name, 0) else ref for ref in user.inputs]
                del g.nodes[rs.name]
        c.refresh()
        if not c.cons.get(last.name):
            del g.nodes[last.name]
            c.refresh()


# ------------------------------------------------------------------ embeddings
class EmbeddingLNOp:
    """LN(sum of row gathers + position rows), the BERT embedding block
    (modeling.py ``embedding_lookup`` / ``embedding_postprocessor``) as one
    ``embed_ln`` launch: one wave per token, tables held in bf16."""

    def __init__(self, tables, pos, seq, gamma, beta, eps, device, use_hip):
        self.seq, self.eps, self.use_hip = int(seq), float(eps), use_hip
        self.tables_f = [t.float().contiguous() for t in tables]
        self.pos_f = None if pos is None else pos.float().reshape(-1, tables[0].shape[1]).contiguous()
        self.g = to_device(gamma.float().reshape(-1), device)
        self.b = to_device(beta.float().reshape(-1), device)
        self.hip_ok = use_hip and device.type == "cuda" and len(tables) <= 2
        if self.hip_ok:
            self.tables = [to_device(t, device, BF16) for t in tables]
            self.pos = None if pos is None else to_device(self.pos_f, device, BF16)
            self.tables_f = self.pos_f = None     # only the bf16 copies stay resident
        else:
            self.tables_f = [to_device(t, device) for t in self.tables_f]
            self.pos_f = None if self.pos_f is None else to_device(self.pos_f, device)

    def __call__(self, ctx, node, ins):
        idx = [O.to_torch(v) for v in ins]
        S = self.seq
        n = idx[0].numel()
        for i in idx[1:]:
            if i.numel() != n:
                raise O.OpError(f"{node.name}: embedding index counts differ")
        if n % S:
            raise O.OpError(f"{node.name}: {n} ids do not reshape to [-1, {S}]")
        if self.hip_ok:
            from ..ops import hip
            dev = self.g.device
            ii = [i.to(dev, torch.int32).reshape(-1).contiguous() for i in idx]
            y = hip().embed_ln(ii[0], ii[1] if len(ii) > 1 else None, self.tables[0], self.pos,
                               self.tables[1] if len(ii) > 1 else None, self.g, self.b, self.eps, S)
            return [y.reshape(-1, S, y.shape[-1])]
        acc = None
        for i, t in zip(idx, self.tables_f):
            i = i.reshape(-1).to(t.device).long()
            if t.device.type == "cpu":
                if n and (int(i.min()) < 0 or int(i.max()) >= t.shape[0]):
                    raise O.OpError(f"{node.name}: indices out of range [0, {t.shape[0]})")
                r = t.index_select(0, i)
            else:
                ok = (i >= 0) & (i < t.shape[0])
                r = t.index_select(0, i.clamp(0, t.shape[0] - 1)) * ok[:, None].float()
            acc = r if acc is None else acc + r
        y = acc.reshape(-1, S, acc.shape[-1])
        if self.pos_f is not None:
            y = y + self.pos_f[:S]
        return [F.layer_norm(y, (y.shape[-1],), self.g, self.b, self.eps)]


def _gather_term(g, c, ref):
    """Reshape(GatherV2(table, idx, 0), [-1, S, Hd]) -> (table, idx_ref, S, nodes)."""
    rs = _node(g, ref)
    if rs is None or rs.op != "Reshape":
        return None
    shp = _const_t(g, rs.inputs[1])
    ga = _node(g, rs.inputs[0])
    if shp is None or ga is None or ga.op != "GatherV2" or int(ga.attr("batch_dims", 0)) != 0:
        return None
    shp = shp.reshape(-1).tolist()
    table, ax = _const_t(g, ga.inputs[0]), _scalar(g, ga.inputs[2])
    if table is None or table.dim() != 2 or ax != 0 or len(shp) != 3 or shp[0] != -1 or shp[2] != table.shape[1]:
        return None
    return table, ga.inputs[1], int(shp[1]), [rs, ga]


def fuse_embedding(g, order, fed, fetch_refs, device, opts):
    """_LayerNorm(word gather + [type gather] + [position rows]) -> _EmbeddingLN."""
    from .fused import _Ctx
    c = _Ctx(g, order, fed, fetch_refs, device, opts)
    for name in order:
        ln = g.nodes.get(name)
        if ln is None or ln.op != "_LayerNorm":
            continue
        leaves, interior, stack = [], [], [ln.inputs[0]]
        while stack and len(leaves) <= 3:
            ref = stack.pop()
            n = _node(g, ref)
            if n is not None and n.op in ("Add", "AddV2") and len(n.inputs) == 2:
                interior.append(n)
                stack += n.inputs
            else:
                leaves.append(ref)
        if not interior or len(leaves) > 3:
            continue
        gathers, pos = [], []
        for ref in leaves:
            gt = _gather_term(g, c, ref)
            if gt is not None:
                gathers.append(gt)
                continue
            v = _const_t(g, ref)
            if v is None:
                break
            pos.append(v)
        else:
            if not gathers or len(pos) > 1:
                continue
            S, Hd = gathers[0][2], gathers[0][0].shape[1]
            if any(gt[2] != S or gt[0].shape[1] != Hd for gt in gathers):
                continue
            p = pos[0] if pos else None
            if p is not None and tuple(p.shape) not in ((1, S, Hd), (S, Hd)):
                continue
            impl = ln.attrs["_impl"]
            if impl.g.numel() not in (1, Hd) or impl.b.numel() not in (1, Hd):
                continue
            ln_g, ln_b = impl.params(Hd)
            nodes = interior + [n for gt in gathers for n in gt[3]]
            if not _interior_ok(c, nodes, ln):
                continue
            gathers.sort(key=lambda gt: -gt[0].shape[0])    # largest (word) table first
            _remove(g, nodes)
            ln.op = "_EmbeddingLN"
            ln.inputs = [gt[1] for gt in gathers]
            ln.ctrl = []
            ln.attrs = {"_impl": EmbeddingLNOp([gt[0] for gt in gathers], p, S, ln_g, ln_b, impl.eps,
                                               device, c.use_hip)}
            c.refresh()


# ------------------------------------------------------------------ attention mask
class KeyMaskAdderOp:
    """(one - X) * scale for a key mask X [B, 1, S], shaped [B, 1, 1, S]: the
    BERT attention adder (modeling.py ``create_attention_mask_from_input_mask``
    + ``(1 - mask) * -10000``) without materialising the [B, S, S] broadcast.
    Only _Attention consumes it, and it broadcasts over the query axis."""

    def __init__(self, one, scale):
        self.one, self.scale = float(one), float(scale)

    def __call__(self, ctx, node, ins):
        x = O.to_torch(ins[0])
        if x.dim() != 3 or x.shape[1] != 1:
            raise O.Unsupported("key mask must be [B, 1, S]")
        if x.is_cuda and x.dtype in (torch.int32, torch.float32):
            from ..ops import hip
            return [hip().key_mask_adder(x.contiguous(), self.one, self.scale).unsqueeze(1)]   # one launch
        return [(x.float() * -self.scale).add_(self.one * self.scale).unsqueeze(1)]


def fuse_key_mask(g, order, fed, fetch_refs, device, opts):
    """Mul(Sub(1, ExpandDims(Mul(ones[1,S,1], X), 1)), c) feeding only _Attention
    nodes -> _KeyMaskAdder(X)."""
    from .fused import _Ctx
    c = _Ctx(g, order, fed, fetch_refs, device, opts)
    for name in order:
        mul = g.nodes.get(name)
        if mul is None or mul.op != "Mul" or len(mul.inputs) != 2 or name in c.fetch_nodes:
            continue
        cons = c.cons.get(name, [])
        if not cons or any(g.nodes[cn].op != "_Attention" or pos != 1 or oi != 0 for cn, pos, oi in cons):
            continue
        for k in (0, 1):
            sub, scale = _node(g, mul.inputs[k]), _scalar(g, mul.inputs[1 - k])
            if sub is not None and sub.op == "Sub" and scale is not None:
                break
        else:
            continue
        one, ex = _scalar(g, sub.inputs[0]), _node(g, sub.inputs[1])
        if one is None or ex is None or ex.op != "ExpandDims" or _scalar(g, ex.inputs[1]) != 1:
            continue
        bm = _node(g, ex.inputs[0])
        if bm is None or bm.op != "Mul" or len(bm.inputs) != 2:
            continue
        x_ref = None
        for k in (0, 1):
            ones = _const_t(g, bm.inputs[k])
            if ones is not None and ones.dim() == 3 and ones.shape[0] == 1 and ones.shape[2] == 1 and \
                    bool((ones == 1).all()):
                x_ref = bm.inputs[1 - k]
                S = ones.shape[1]
        if x_ref is None or not _interior_ok(c, [sub, ex, bm], mul):
            continue
        interior = [sub, ex, bm]
        cast = _node(g, x_ref)
        if cast is not None and cast.op == "Cast" and not cast.ctrl and \
                O.dt_attr(cast, "DstT") == torch.float32 and _interior_ok(c, interior + [cast], mul):
            interior.append(cast)        # the op casts to f32 itself
            x_ref = cast.inputs[0]
        _remove(g, interior)
        mul.op = "_KeyMaskAdder"
        mul.inputs = [x_ref]
        mul.ctrl = []
        mul.attrs = {"_impl": KeyMaskAdderOp(one, scale), "_seq": S}
        c.refresh()


# ------------------------------------------------------------------ DLRM: embedding bags, dot interaction
class EmbeddingBagOp:
    """``Pack([x_0?, e_0 .. e_{F-1}], axis=1)`` (or ``Reshape(ConcatV2(.., axis=1), [-1, F0 + F, D])``)
    with ``e_f = Sum(GatherV2(table_f, ids_f, axis 0), axis=1)``: on the GPU one ``embedding_bag``
    launch (kernels/embag.hip) from one bf16 blob of all tables, rounded once here from the fp32
    variables as EmbeddingLNOp holds its tables.  ``split``: the id tensors were the outputs of one
    ``SplitV(sparse, sizes, axis=1)``, and the op reads ``sparse [B, T]`` itself; otherwise it takes
    the F id tensors ``[B, L_f]`` and concatenates them on the device.  The CPU, and any input the
    kernel does not take, get the replaced nodes' own semantics from torch; on the CPU an id outside
    its table raises as the interpreter's GatherV2 does, on the device it adds a zero row (a select,
    never a product: the clamped row may hold Inf)."""

    def __init__(self, tables, split, lead: bool, concat: bool, device, use_hip: bool, name: str):
        self.vocab = [int(t.shape[0]) for t in tables]
        self.d = int(tables[0].shape[1])
        self.split = None if split is None else [int(s) for s in split]
        self.lead, self.concat = bool(lead), bool(concat)
        self.use_hip = use_hip
        self.name = name
        self.base = [sum(self.vocab[:f]) for f in range(len(tables))]
        blob = torch.cat([t.reshape(v, self.d) for t, v in zip(tables, self.vocab)], dim=0)
        self.blob = to_device(blob, device, BF16 if use_hip else torch.float32)
        self._feat = {}                 # hotness tuple -> (flat host list, device [F, 4] int64)
        if use_hip and self.split is not None and self.blob.is_cuda:
            self.features(self.split, self.blob.device)

    def features(self, hot, device):
        """(row base, V, first slot, hotness) per feature: the flat host list the binding checks
        and the device array the kernel reads (cached per hotness tuple: built before any capture
        when the ids come from a SplitV, whose sizes are constants)."""
        key = (tuple(hot), str(device))
        if key not in self._feat:
            flat, first = [], 0
            for base, v, l in zip(self.base, self.vocab, hot):
                flat += [base, v, first, int(l)]
                first += int(l)
            self._feat[key] = (flat, torch.tensor(flat, dtype=torch.int64).view(-1, 4).to(device))
        return self._feat[key]

    def _rows(self, node, f: int, idx: torch.Tensor) -> torch.Tensor:
        """Sum(GatherV2(table_f, idx, axis 0), axis=1) in fp32."""
        base, v = self.base[f], self.vocab[f]
        flat = idx.reshape(-1).to(self.blob.device).long()
        if flat.device.type == "cpu":
            if flat.numel() and (int(flat.min()) < 0 or int(flat.max()) >= v):
                raise O.OpError(f"{node.name}: indices out of range [0, {v})")
            rows = self.blob.index_select(0, flat + base).float()
        else:
            ok = (flat >= 0) & (flat < v)
            rows = self.blob.index_select(0, flat.clamp(0, v - 1) + base).float()
            rows = torch.where(ok[:, None], rows, torch.zeros((), dtype=rows.dtype, device=rows.device))
        g = rows.reshape(list(idx.shape) + [self.d])
        if g.dim() < 2:
            raise O.OpError(f"{node.name}: cannot sum a rank-{g.dim()} gather over axis 1")
        return g.sum(dim=1)

    def __call__(self, ctx, node, ins):
        ins = [O.to_torch(v) for v in ins]
        lead = ins[0] if self.lead else None
        ids = ins[1:] if self.lead else ins
        if self.use_hip and self.blob.is_cuda and all(i.is_cuda and i.dim() == 2 and i.dtype in (torch.int32, torch.int64)
                                                      for i in ids):
            from ..ops import hip
            from .fused import _to_bf16
            H = hip()
            if self.split is not None:
                sparse, hot = ids[0], self.split
            else:
                hot = [int(i.shape[1]) for i in ids]
                same = all(i.shape[0] == ids[0].shape[0] and i.dtype == ids[0].dtype for i in ids)
                sparse = torch.cat(ids, dim=1) if same and all(1 <= l for l in hot) else None
            if sparse is not None and sparse.shape[1] == sum(hot):
                B, T = int(sparse.shape[0]), int(sparse.shape[1])
                lead_ok = lead is None or (lead.is_cuda and lead.dim() == 2 and tuple(lead.shape) == (B, self.d) and
                                           lead.is_floating_point())
                flat, feat = self.features(hot, sparse.device)
                if lead_ok and H.embedding_bag_supported(B, T, self.d, flat, int(self.blob.shape[0]), lead is not None,
                                                         sparse.dtype == torch.int64):
                    dense = None if lead is None else _to_bf16(lead).contiguous()
                    return [H.embedding_bag(sparse.contiguous(), self.blob, feat, flat, dense)]
        if self.split is not None:
            x = ids[0]
            if x.dim() < 2:
                raise O.OpError(f"{node.name}: cannot split a rank-{x.dim()} tensor along axis 1")
            ids = list(torch.split(x, self.split, dim=1))       # (a wrong width raises, as the SplitV did)
        parts = [self._rows(node, f, i) for f, i in enumerate(ids)]
        if lead is not None:
            parts = [lead.float().to(parts[0].device)] + parts
        if self.concat:
            y = torch.cat(parts, dim=1).reshape(-1, len(parts), self.d)
        else:
            y = torch.stack(parts, dim=1)
        return [y.to(BF16) if self.use_hip and y.is_cuda else y]


def _bag_term(g, c, ref, reader: Node):
    """``ref`` = Sum(GatherV2(table const [V, D], ids, axis 0, batch_dims 0), axis=1, keep_dims=False),
    both read once (the Sum by ``reader``) and not fetched -> (table, ids ref, [sum, gather]) or None."""
    s = _node(g, ref)
    if s is None or s.op != "Sum" or len(s.inputs) != 2 or bool(s.attr("keep_dims", False)) or \
            c.only_consumer(s.name) is not reader:
        return None
    ax = _const_t(g, s.inputs[1])
    if ax is None or ax.numel() != 1 or ax.is_floating_point() or int(ax.reshape(-1)[0]) != 1:
        return None
    ga = _node(g, s.inputs[0])
    if ga is None or ga.op != "GatherV2" or len(ga.inputs) != 3 or int(ga.attr("batch_dims", 0)) != 0 or \
            c.only_consumer(ga.name) is not s:
        return None
    table, gax = _const_t(g, ga.inputs[0]), _const_t(g, ga.inputs[2])
    if table is None or table.dim() != 2 or not table.is_floating_point() or table.shape[0] < 1 or table.shape[1] < 1:
        return None
    if gax is None or gax.numel() != 1 or gax.is_floating_point() or int(gax.reshape(-1)[0]) != 0:
        return None
    if _const_t(g, ga.inputs[1]) is not None:
        return None
    return table, ga.inputs[1], [s, ga]


def _common_split(g, c, id_refs, gathers):
    """The ``SplitV(sparse, const size_splits, axis=1)`` whose outputs 0 .. F-1, in order, are
    ``id_refs`` and feed nothing else -> (split node, sizes) or None."""
    sp = g.nodes.get(id_refs[0][0])
    if sp is None or sp.op != "SplitV" or len(sp.inputs) != 3 or sp.name in c.fetch_nodes:
        return None
    if [tuple(r) for r in id_refs] != [(sp.name, f) for f in range(len(id_refs))]:
        return None
    sizes, ax = _const_t(g, sp.inputs[1]), _const_t(g, sp.inputs[2])
    if sizes is None or ax is None or ax.numel() != 1 or int(ax.reshape(-1)[0]) != 1 or sizes.is_floating_point():
        return None
    sizes = [int(v) for v in sizes.reshape(-1).tolist()]
    if len(sizes) != len(id_refs) or any(s < 1 for s in sizes):
        return None
    readers = sorted(cn for cn, _p, _i in c.cons.get(sp.name, []))
    if readers != sorted(ga.name for ga in gathers):
        return None
    return sp, sizes


def fuse_embedding_bag(g, order, fed, fetch_refs, device, opts):
    """``Pack([x_0?, e_0 .. e_{F-1}], axis=1)`` and ``Reshape(ConcatV2([..], axis=1), [-1, F0 + F, D])``
    with every ``e_f`` a pooled row gather (``_bag_term``) of one width D, behind at most one leading
    operand that is none -> ``_EmbeddingBag(x_0?, ids..)`` (class EmbeddingBagOp).  When the id
    tensors are the outputs of one SplitV in order, the op reads its input and the SplitV goes."""
    from .fused import _Ctx
    c = _Ctx(g, order, fed, fetch_refs, device, opts)
    for name in order:
        out = g.nodes.get(name)
        if out is None:
            continue
        concat = None
        if out.op == "Pack" and int(out.attr("axis", 0)) == 1:
            reader, operands = out, list(out.inputs)
        elif out.op == "Reshape" and len(out.inputs) == 2:
            concat = _node(g, out.inputs[0])
            if concat is None or concat.op != "ConcatV2" or len(concat.inputs) < 2 or \
                    c.only_consumer(concat.name) is not out:
                continue
            ax = _const_t(g, concat.inputs[-1])
            if ax is None or ax.numel() != 1 or int(ax.reshape(-1)[0]) != 1:
                continue
            reader, operands = concat, list(concat.inputs[:-1])
        else:
            continue
        if not operands:
            continue
        terms = [_bag_term(g, c, r, reader) for r in operands]
        lead = terms[0] is None
        if lead:
            terms = terms[1:]
        if not terms or any(t is None for t in terms):
            continue
        D = int(terms[0][0].shape[1])
        if any(int(t[0].shape[1]) != D for t in terms):
            continue
        if concat is not None:
            shp = _const_t(g, out.inputs[1])
            if shp is None or [int(v) for v in shp.reshape(-1).tolist()] != [-1, len(operands), D]:
                continue
        id_refs = [t[1] for t in terms]
        gathers = [t[2][1] for t in terms]
        split = _common_split(g, c, id_refs, gathers)
        interior = [n for t in terms for n in t[2]] + ([concat] if concat is not None else [])
        impl = EmbeddingBagOp([t[0] for t in terms], None if split is None else split[1], lead, concat is not None,
                              device, c.use_hip, out.name)
        ins = ([operands[0]] if lead else []) + ([split[0].inputs[0]] if split is not None else id_refs)
        if split is not None:
            interior.append(split[0])
        ctrl = []
        for n in interior + [out]:
            ctrl += [x for x in n.ctrl if x not in ctrl]
        _remove(g, interior)
        out.op = "_EmbeddingBag"
        out.inputs = ins
        out.ctrl = [x for x in ctrl if x in g.nodes]
        out.attrs = {"_impl": impl}
        out.value = None
        c.refresh()


def tril_pairs(f: int, k: int) -> List[int]:
    """``i * f + j`` over ``np.tril_indices(f, k)`` (row-major: i ascending, then j <= i + k)."""
    return [i * f + j for i in range(f) for j in range(0, min(i + k, f - 1) + 1)]


class DotInteractionOp:
    """``[Pad(] ConcatV2([dense, GatherV2(Reshape(BatchMatMul(Z, Z, adj_y), [-1, F F]), idx, axis=1)], axis=1)
    [, [[0, 0], [0, pad]])]`` with ``idx`` the strict (``self_interaction`` False) or full lower
    triangle in ``np.tril_indices`` order: on the GPU one ``dot_interaction`` launch
    (kernels/interact.hip), fp32 accumulate and one rounding; the CPU and any input the kernel does
    not take get the replaced nodes' semantics from torch."""

    def __init__(self, f: int, self_interaction: bool, pad: int, device, use_hip: bool, name: str):
        self.f, self.self_interaction, self.pad = int(f), bool(self_interaction), int(pad)
        self.use_hip = use_hip
        self.name = name
        self.idx = to_device(torch.tensor(tril_pairs(self.f, 0 if self_interaction else -1), dtype=torch.int64), device)

    def __call__(self, ctx, node, ins):
        z, dense = O.to_torch(ins[0]), O.to_torch(ins[1])
        nf = self.f
        P = int(self.idx.numel())
        if (self.use_hip and z.is_cuda and z.dim() == 3 and z.shape[1] == nf and z.is_floating_point() and
                dense.is_cuda and dense.dim() == 2 and dense.shape[0] == z.shape[0] and dense.is_floating_point() and
                dense.shape[1] >= 8):
            from ..ops import hip
            from .fused import _to_bf16
            H = hip()
            B, D, Dd = int(z.shape[0]), int(z.shape[2]), int(dense.shape[1])
            if H.dot_interaction_supported(B, nf, D, Dd, self.pad, self.self_interaction):
                y = H.dot_interaction(_to_bf16(z).contiguous(), _to_bf16(dense).contiguous(), self.self_interaction,
                                      self.pad)
                w = Dd + P + self.pad
                return [y if y.shape[1] == w else y[:, :w]]
        zf = z.float()
        if zf.dim() < 2:
            raise O.OpError(f"{node.name}: BatchMatMul of a rank-{zf.dim()} tensor")
        zz = torch.matmul(zf, zf.transpose(-1, -2))
        try:
            flat = zz.reshape(-1, nf * nf)
        except RuntimeError as e:
            raise O.OpError(f"{node.name}: cannot reshape {list(zz.shape)} to [-1, {nf * nf}]: {e}") from None
        pairs = flat.index_select(1, self.idx.to(flat.device))
        y = torch.cat([dense.float().to(pairs.device), pairs], dim=1)
        if self.pad:
            y = F.pad(y, [0, self.pad])
        return [y.to(BF16) if self.use_hip and y.is_cuda else y]


def fuse_dot_interaction(g, order, fed, fetch_refs, device, opts):
    """The pattern of class DotInteractionOp -> ``_DotInteraction(Z, dense)``.  Constants are read
    by shape: ``idx`` must equal ``i F + j`` over ``np.tril_indices(F, -1)`` or ``(F, 0)`` exactly,
    with F from the reshape's ``[-1, F F]``; the BatchMatMul has one operand twice, ``adj_y`` and no
    ``adj_x``; a Pad is taken only as ``[[0, 0], [0, p]]`` with zeros.  The gather, the reshape, the
    product and a concat that feeds a taken Pad are read once and not fetched."""
    from .fused import _Ctx
    c = _Ctx(g, order, fed, fetch_refs, device, opts)
    for name in order:
        cat = g.nodes.get(name)
        if cat is None or cat.op != "ConcatV2" or len(cat.inputs) != 3:
            continue
        ax = _const_t(g, cat.inputs[2])
        if ax is None or ax.numel() != 1 or ax.is_floating_point() or int(ax.reshape(-1)[0]) != 1:
            continue
        ga = _node(g, cat.inputs[1])
        if ga is None or ga.op != "GatherV2" or len(ga.inputs) != 3 or int(ga.attr("batch_dims", 0)) != 0 or \
                c.only_consumer(ga.name) is not cat:
            continue
        idx, gax = _const_t(g, ga.inputs[1]), _const_t(g, ga.inputs[2])
        if idx is None or idx.is_floating_point() or idx.dim() != 1 or gax is None or gax.numel() != 1 or \
                gax.is_floating_point() or int(gax.reshape(-1)[0]) != 1:
            continue
        rs = _node(g, ga.inputs[0])
        if rs is None or rs.op != "Reshape" or len(rs.inputs) != 2 or c.only_consumer(rs.name) is not ga:
            continue
        shp = _const_t(g, rs.inputs[1])
        if shp is None or shp.numel() != 2 or int(shp.reshape(-1)[0]) != -1:
            continue
        ff = int(shp.reshape(-1)[1])
        f = math.isqrt(ff) if ff > 0 else 0
        if f < 2 or f * f != ff:
            continue
        bm = _node(g, rs.inputs[0])
        if bm is None or bm.op not in ("BatchMatMul", "BatchMatMulV2", "BatchMatMulV3") or len(bm.inputs) != 2 or \
                bm.inputs[0] != bm.inputs[1] or bool(bm.attr("adj_x", False)) or not bool(bm.attr("adj_y", False)) or \
                c.only_consumer(bm.name) is not rs or _const_t(g, bm.inputs[0]) is not None:
            continue
        got = [int(v) for v in idx.tolist()]
        if got == tril_pairs(f, -1):
            self_int = False
        elif got == tril_pairs(f, 0):
            self_int = True
        else:
            continue
        interior, last, pad = [ga, rs, bm], cat, 0
        p = c.only_consumer(cat.name)
        if p is not None and p.op in ("Pad", "PadV2") and p.inputs[0] == (cat.name, 0):
            pv = _const_t(g, p.inputs[1])
            zero = p.op == "Pad" or (_scalar(g, p.inputs[2]) == 0.0)
            if pv is not None and tuple(pv.shape) == (2, 2) and not pv.is_floating_point() and zero:
                (b0, b1), (c0, c1) = pv.tolist()
                if b0 == 0 and b1 == 0 and c0 == 0 and c1 >= 0:
                    interior, last, pad = interior + [cat], p, int(c1)
        impl = DotInteractionOp(f, self_int, pad, device, c.use_hip, last.name)
        ctrl = []
        for n in interior + [last]:
            ctrl += [x for x in n.ctrl if x not in ctrl]
        z_ref, dense_ref = bm.inputs[0], cat.inputs[0]
        _remove(g, interior)
        last.op = "_DotInteraction"
        last.inputs = [z_ref, dense_ref]
        last.ctrl = [x for x in ctrl if x in g.nodes]
        last.attrs = {"_impl": impl}
        last.value = None
        c.refresh()


def dlrm_passes():
    """TFSERVE_DLRM=0 (read at every compile) removes the two passes: scripts/dlrm_bench.py's A/B in one build."""
    return [] if os.environ.get("TFSERVE_DLRM", "1") == "0" else [fuse_embedding_bag, fuse_dot_interaction]


def bert_passes():
    return [fuse_layernorm, fuse_embedding, fuse_window_attention, fold_window_layout, fuse_attention, fuse_key_mask]


def late_passes():
    """Passes over the fused graph (after every GEMM is a _FusedMatMul).  None
    here; the LayerNorm fold runs last (graph/fused.py defer_layernorm: round
    3's fold spilled registers in the 8-wave tiles and was removed in round 4,
    profiles/round3/ln_fold.md; round 5's epilogue reads its per-column
    vectors from LDS instead)."""
    return []
