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

* GPT-2's causal attention (``fuse_causal_attention``): the mask spelled ``w * b - fill * (1 - b)`` or
  ``SelectV2(b, w, fill)`` over the lower-triangular band b, q / k / v from one packed dense
        => _FusedQKV(x)  ->  _CausalAttention(qkv, key_adder)

* Llama's block (``fuse_rmsnorm``, ``fuse_rope_attention``, ``fuse_swiglu``): RMSNorm spelled ``Square`` / ``Mean`` /
  ``Rsqrt``, the causal core with q and k rotated by position and k / v repeated for their group of query heads,
  and ``swish(x Wg) * (x Wu)``
        => _RMSNorm(x [, residual])   _FusedQKV(x) -> _RopeGQAttention(qkv, key_adder)   _FusedMatMul -> _SwiGLU

* ModernBERT's block (``fuse_rope_encoder_attention``, ``fuse_geglu``): the bidirectional core with q and k rotated by
  position and an optional constant local band ``fill * (|i - j| > w)`` added to the scores, and
  ``gelu_erf(s0) * s1`` over the two halves of one dense
        => _FusedQKV(x) -> _RopeAttention(qkv, key_adder; window)   _FusedMatMul -> _GeGLU

* T5's encoder attention (``fuse_bias_attention``): the bidirectional core with one constant per-head bias that is
  exactly Toeplitz (a function of j - i: the relative-position bias) and an optional adder, in either nesting
        => _FusedQKV(x) -> _BiasAttention(qkv, key_adder; table [H, 2 S - 1])

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


# ------------------------------------------------------------------ causal attention (GPT-2)
MIN_CAUSAL_FILL = 1e4         # a smaller |fill| leaves a masked key a visible share of the softmax


class CausalAttentionOp:
    """softmax(mask(q k^T * scale) (+ adder)) v over a packed QKV buffer, mask =
    keep the score where key <= query, else ``closed`` (the matched graph's
    ``-fill`` of ``w * b - fill * (1 - b)``, or the ``fill`` of ``SelectV2``).

    On the device, for D = 64 and an adder that is absent or [B | 1, 1, 1, S],
    one ``causal_attention`` launch (kernels/cattn.hip), which closes masked
    keys with -inf instead of ``closed``: equal to rounding wherever a row has
    an open key whose adder is 0 (docs/numerics.md, "Causal attention").
    Anywhere else the graph's own arithmetic with torch, in fp32."""

    def __init__(self, heads: int, head_dim: int, seq: int, scale: float, closed: float, use_hip: bool):
        self.h, self.d, self.s, self.scale, self.closed, self.use_hip = heads, head_dim, seq, scale, closed, use_hip

    def __call__(self, ctx, node, ins):
        qkv = O.to_torch(ins[0])
        adder = O.to_torch(ins[1]) if len(ins) > 1 else None
        S, H, D = self.s, self.h, self.d
        if qkv.numel() % (S * 3 * H * D):
            raise O.OpError(f"{node.name}: {list(qkv.shape)} is not [B * {S}, {3 * H * D}]")
        B = qkv.numel() // (S * 3 * H * D)
        key_adder = adder is None or (adder.dim() == 4 and tuple(adder.shape[1:]) == (1, 1, S) and
                                      adder.shape[0] in (1, B))
        if self.use_hip and qkv.is_cuda and D == 64 and 1 <= S <= MAX_ATTENTION_SEQ and key_adder:
            from ..ops import hip
            from .fused import _to_bf16
            q3 = _to_bf16(qkv).reshape(B, S, 3 * H * D).contiguous()
            ka = None if adder is None else adder.float().reshape(-1, S).contiguous().to(qkv.device)
            return [hip().causal_attention(q3, ka, H, self.scale).reshape(B * S, H * D)]
        q, k, v = qkv.float().reshape(B, S, 3, H, D).permute(2, 0, 3, 1, 4)
        sc = q @ k.transpose(-1, -2) * self.scale
        band = torch.ones(S, S, dtype=torch.bool, device=sc.device).tril()
        sc = torch.where(band, sc, torch.full_like(sc, self.closed))
        if adder is not None:
            sc = sc + adder.float().to(sc.device)
        y = (torch.softmax(sc, -1) @ v).permute(0, 2, 1, 3).reshape(B * S, H * D)
        return [y if not qkv.is_cuda else y.to(qkv.dtype)]


def _square(v: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    """A constant shaped [S, S] under at most two leading 1s -> it as [S, S], else None."""
    if v is None or v.dim() < 2 or v.dim() > 4 or v.shape[-1] != v.shape[-2] or v.numel() != v.shape[-1] ** 2:
        return None
    return v.reshape(v.shape[-1], v.shape[-1])


def _causal_mask(g, n: Optional[Node]):
    """n = Sub(Mul(w, b), c) or SelectV2(b, w, fill) with b the exact lower-triangular band
    -> (w ref, S, the value of a masked score, nodes), else None."""
    m = _masked_scores(g, n)
    if m is None or not torch.equal(m[1].double(), torch.ones(m[1].shape, dtype=torch.float64).tril()):
        return None
    return m[0], int(m[1].shape[0]), m[2], m[3]


def _window_mask(g, n: Optional[Node]):
    """``_causal_mask`` for a sliding window: b's ones are exactly {0 <= i - j <= w} for one integer w >= 0
    -> (w ref, S, the value of a masked score, nodes, window), window = -1 when the band is the whole
    triangle (w >= S - 1), else None.  w is read off column 0, then the whole matrix is compared: a hole, a
    band off the diagonal, an upper band or two widths in one band are not a window."""
    m = _masked_scores(g, n)
    if m is None:
        return None
    b = m[1].double()
    S = int(b.shape[0])
    w = int(b[:, 0].sum()) - 1
    pos = torch.arange(S)
    d = pos[:, None] - pos[None, :]
    if w < 0 or not torch.equal(b, ((d >= 0) & (d <= w)).double()):
        return None
    return m[0], S, m[2], m[3], (w if w < S - 1 else -1)


def _masked_scores(g, n: Optional[Node]):
    """n = Sub(Mul(w, b), c) or SelectV2(b, w, fill) with b a constant 0/1 (or bool) [S, S] under leading 1s,
    c = fill * (1 - b), fill strong enough -> (w ref, b, the value of a masked score, nodes), else None.
    What b's ones must be is the caller's question."""
    if n is None:
        return None
    if n.op == "SelectV2" and len(n.inputs) == 3:
        b, fill = _square(_const_t(g, n.inputs[0])), _const_t(g, n.inputs[2])
        if b is None or b.dtype != torch.bool or fill is None or fill.numel() != 1 or not fill.is_floating_point():
            return None
        closed, w_ref, nodes = float(fill), n.inputs[1], [n]
        if not closed <= -MIN_CAUSAL_FILL:
            return None
    elif n.op == "Sub" and len(n.inputs) == 2:
        mul, cv = _node(g, n.inputs[0]), _square(_const_t(g, n.inputs[1]))
        if mul is None or mul.op != "Mul" or len(mul.inputs) != 2 or cv is None or not cv.is_floating_point():
            return None
        for k in (0, 1):
            b = _square(_const_t(g, mul.inputs[k]))
            if b is not None:
                break
        else:
            return None
        if not b.is_floating_point() or b.shape != cv.shape:
            return None
        # c = fill * (1 - b): zero on the band, one value everywhere above it
        fill = float(cv[0, -1]) if cv.shape[0] > 1 else MIN_CAUSAL_FILL
        if not fill >= MIN_CAUSAL_FILL or not torch.equal(cv.double(), fill * (1.0 - b.double())):
            return None
        closed, w_ref, nodes = -fill, mul.inputs[1 - k], [n, mul]
    else:
        return None
    return w_ref, b, closed, nodes


def _split_qkv(g, c, refs, H: int, D: int):
    """refs = outputs 0, 1, 2 of Split(axis = last, num_split = 3) | SplitV(equal sizes) over
    [Reshape of] one dense 3 * H * D wide -> (x ref, w, b, nodes), else None."""
    sp = g.nodes.get(refs[0][0])
    if sp is None or list(refs) != [(sp.name, 0), (sp.name, 1), (sp.name, 2)]:
        return None
    if sp.op == "Split" and len(sp.inputs) == 2 and int(sp.attr("num_split", 0)) == 3:
        axis, src = _ints(g, sp.inputs[0]), sp.inputs[1]
    elif sp.op == "SplitV" and len(sp.inputs) == 3 and _ints(g, sp.inputs[1]) == [H * D] * 3:
        axis, src = _ints(g, sp.inputs[2]), sp.inputs[0]
    else:
        return None
    nodes, rank = [sp], 2
    r = _node(g, src)
    if r is not None and r.op == "Reshape":
        shp = _ints(g, r.inputs[1])
        if shp is None or not shp or shp[-1] != 3 * H * D:
            return None
        nodes.append(r)
        rank, src = len(shp), r.inputs[0]
    if axis is None or len(axis) != 1 or axis[0] not in (-1, rank - 1):
        return None
    ds = _dense_src(g, c, src)
    if ds is None or ds[1].shape[1] != 3 * H * D:
        return None
    return ds[0], ds[1], ds[2], nodes + ds[3]


def _causal_core(g, out: Node, mask_of=None):
    """out = Reshape(Transpose(BatchMatMul(Softmax(scores), v), [0, 2, 1, 3]), .) with ``scores`` the causally
    masked, optionally scaled q k^T of fuse_causal_attention, with or without an adder
    -> (qk node, pv node, S, scale, closed, adder ref | None, interior nodes, window), else None.
    ``mask_of`` is ``_causal_mask`` (the default: window is -1) or ``_window_mask``."""
    mask_of = mask_of or _causal_mask
    t2 = _node(g, out.inputs[0])
    if t2 is None or t2.op != "Transpose" or _ints(g, t2.inputs[1]) != [0, 2, 1, 3]:
        return None
    pv = _node(g, t2.inputs[0])
    if pv is None or pv.op not in _BMM or pv.attr("adj_x", False) or pv.attr("adj_y", False):
        return None
    sm = _node(g, pv.inputs[0])
    if sm is None or sm.op != "Softmax":
        return None
    interior = [t2, pv, sm]
    cur = _node(g, sm.inputs[0])
    adder_ref = None
    if cur is not None and cur.op in ("Add", "AddV2") and len(cur.inputs) == 2:
        for k in (0, 1):
            side = _node(g, cur.inputs[k])
            if side is not None and side.op in ("Sub", "SelectV2") and mask_of(g, side) is not None:
                break
        else:
            return None
        adder_ref = cur.inputs[1 - k]
        interior.append(cur)
        cur = side
    cm = mask_of(g, cur)
    if cm is None:
        return None
    w_ref, S, closed, nodes = cm[:4]
    window = cm[4] if len(cm) > 4 else -1
    interior += nodes
    scale = 1.0
    qk = _node(g, w_ref)
    sv = _scale_of(g, qk) if qk is not None and qk.op in ("Mul", "RealDiv") else None
    if sv is not None:
        scale = sv[0]
        interior.append(qk)
        qk = _node(g, sv[1])
    if qk is None or qk.op not in _BMM or qk.attr("adj_x", False) or not qk.attr("adj_y", False):
        return None
    interior.append(qk)
    return qk, pv, S, scale, closed, adder_ref, interior, window


def fuse_causal_attention(g, order, fed, fetch_refs, device, opts):
    """GPT-2's attention core -> _FusedQKV -> _CausalAttention::

        w = BatchMatMul(q, k, adj_y)  [Mul by c | RealDiv by c: _scale_of]
        masked = Sub(Mul(w, b), c)            b the constant lower-triangular 0/1 band [S, S] under leading 1s,
               | SelectV2(b, w, fill)         c = fill * (1 - b) with fill >= 1e4  |  b bool, scalar fill <= -1e4
        scores = masked | AddV2(masked, adder)                      (adder: anything but the pattern's own nodes)
        y = Reshape(Transpose(BatchMatMul(Softmax(scores), v), [0, 2, 1, 3]), [-1, H * D])

    q, k, v from three denses on one input (``_heads_of`` + ``_dense_src``) or
    from one dense split three ways (``_split_qkv``).  Runs before
    fuse_attention and takes nothing it takes: that pass has no Sub or SelectV2
    under the Softmax, and a constant [1, 1, S, S] adder added to the scores stays
    its ``_Attention``.  Anything that is not exactly the band (upper-triangular,
    a hole, offset by one, another S), a weaker fill, a ``c`` that is not
    fill * (1 - b), or an interior node read elsewhere is left alone."""
    from .fused import FusedMatMul, _Ctx
    c = _Ctx(g, order, fed, fetch_refs, device, opts)
    for name in list(order):
        out = g.nodes.get(name)
        if out is None or out.op != "Reshape":
            continue
        core = _causal_core(g, out)
        if core is None:
            continue
        qk, pv, S, scale, closed, adder_ref, interior, _window = core
        hq, hk, hv = _heads_of(g, c, qk.inputs[0]), _heads_of(g, c, qk.inputs[1]), _heads_of(g, c, pv.inputs[1])
        if hq is None or hk is None or hv is None or hq[1:4] != hk[1:4] or hq[1:4] != hv[1:4]:
            continue
        H, D = hq[2], hq[3]
        if hq[1] != S or _ints(g, out.inputs[1]) != [-1, H * D]:
            continue                  # (the op returns [B * S, H * D])
        interior += hq[4] + hk[4] + hv[4]
        if adder_ref is not None and adder_ref[0] in {n.name for n in interior}:
            continue
        packed = _split_qkv(g, c, [hq[0], hk[0], hv[0]], H, D)
        if packed is not None:
            x_ref, w, b, qkv_nodes = packed
        else:
            dq, dk, dv = _dense_src(g, c, hq[0]), _dense_src(g, c, hk[0]), _dense_src(g, c, hv[0])
            if not (dq and dk and dv and dq[0] == dk[0] == dv[0]) or any(d[1].shape[1] != H * D for d in (dq, dk, dv)):
                continue
            x_ref = dq[0]
            w = torch.cat([dq[1], dk[1], dv[1]], dim=1)
            b = torch.cat([dq[2], dk[2], dv[2]])
            qkv_nodes = dq[3] + dk[3] + dv[3]
        if not _interior_ok(c, interior + qkv_nodes, out):
            continue
        qkv_name = g.unique_name(out.name + "/fused_qkv")
        g.add(Node(name=qkv_name, op="_FusedQKV", inputs=[x_ref],
                   attrs={"_impl": FusedMatMul(w, b, "none", False, device, c.use_hip, qkv_name)}))
        _remove(g, interior + qkv_nodes)
        out.op = "_CausalAttention"
        out.inputs = [(qkv_name, 0)] + ([adder_ref] if adder_ref is not None else [])
        out.ctrl = []
        out.attrs = {"_impl": CausalAttentionOp(H, D, S, scale, closed, c.use_hip)}
        c.refresh()


# ------------------------------------------------------------------ Llama: RMSNorm, RoPE + GQA attention, SwiGLU
ROPE_GROUPS = (1, 2, 4, 8)    # kernels/launch.h rope_gqa_attention_supported: heads / kv_heads
ROPE_HEAD_DIMS = (64, 128)    # ... and head widths (gqattn.hip, gqattn128.hip)


class RMSNormOp:
    """y = z * rsqrt(mean(z^2) + eps) * gamma over the last axis, z = x or, with two
    inputs, x + r; then the outputs are (y, z).  On the device one ``rmsnorm``
    launch (kernels/llama.hip) for C % 8 == 0, else the graph's arithmetic in fp32."""

    def __init__(self, gamma, eps, device, use_hip):
        self.eps, self.use_hip = float(eps), use_hip
        self.g = to_device(gamma.float().reshape(-1).contiguous(), device)

    def __call__(self, ctx, node, ins):
        x = O.to_torch(ins[0])
        r = O.to_torch(ins[1]) if len(ins) > 1 else None
        cols = x.shape[-1]
        if self.use_hip and x.is_cuda and cols % 8 == 0 and cols == self.g.numel() and \
                (r is None or r.shape == x.shape):
            from ..ops import hip
            from .fused import _to_bf16
            xb = _to_bf16(x).contiguous()
            if r is None:
                return [hip().rmsnorm(xb, self.g, self.eps)]
            z = torch.empty_like(xb)
            return [hip().rmsnorm(xb, self.g, self.eps, _to_bf16(r).contiguous(), None, z), z]
        z = x.float() if r is None else x.float() + r.float().to(x.device)
        y = z * torch.rsqrt((z * z).mean(-1, keepdim=True) + self.eps) * self.g.to(x.device)
        outs = [y] if r is None else [y, z]
        return outs if not x.is_cuda else [o.to(x.dtype) for o in outs]


class SwiGLUOp:
    """swish(gu[:, :F]) * gu[:, F:] after one GEMM over [W_gate | W_up]: ``swiglu``
    (kernels/llama.hip) on the device for F % 8 == 0, else torch in fp32."""

    def __init__(self, width: int, use_hip: bool):
        self.f, self.use_hip = width, use_hip

    def __call__(self, ctx, node, ins):
        gu = O.to_torch(ins[0])
        F_ = self.f
        if gu.shape[-1] != 2 * F_:
            raise O.OpError(f"{node.name}: {list(gu.shape)} is not [M, {2 * F_}]")
        if self.use_hip and gu.is_cuda and F_ % 8 == 0:
            from ..ops import hip
            from .fused import _to_bf16
            y = hip().swiglu(_to_bf16(gu).reshape(-1, 2 * F_).contiguous())
            return [y.reshape(list(gu.shape[:-1]) + [F_])]
        gf = gu.float()
        gate, up = gf[..., :F_], gf[..., F_:]
        y = gate * torch.sigmoid(gate) * up
        return [y if not gu.is_cuda else y.to(gu.dtype)]


class RopeGQAttentionOp:
    """Causal attention over a packed [Q heads | K heads | V heads] buffer with
    q and k rotated by position (rotate-half, tables ``cos`` / ``sin`` [S, D / 2])
    and query head h reading K / V head h / G, G = heads / kv_heads; the mask and
    the adder as in CausalAttentionOp.

    On the device, for D in {64, 128}, G in {1, 2, 4, 8} and an adder that is
    absent or [B | 1, 1, 1, S], one ``rope_gqa_attention`` launch (kernels/gqattn.hip
    for 64-wide heads, kernels/gqattn128.hip for 128-wide ones): it rotates in fp32 and rounds to bf16 once, and closes masked keys with
    -inf (docs/numerics.md, "RoPE + GQA attention").  Anywhere else the graph's
    own arithmetic with torch, in fp32.

    ``qk_norm`` = (q_gamma [D], k_gamma [D], eps): each head's q row and k row is
    RMS-normalised before its rotation (Qwen3).  The launch takes it for D = 128
    (docs/numerics.md, "QK-norm"); 64-wide heads take the torch path.

    ``window`` >= 0 (Gemma's local layers): key j is open for query i iff
    0 <= i - j <= window; -1 is plain causal.  D = 256 takes one
    ``rope_gqa_attention256`` launch (kernels/gqattn256.hip) with or without a
    norm and with any window (docs/numerics.md, "RoPE + GQA attention, D = 256");
    a window at D in {64, 128} takes the torch path."""

    def __init__(self, heads, kv_heads, head_dim, seq, scale, closed, cos, sin, device, use_hip, qk_norm=None,
                 window=-1):
        self.h, self.hkv, self.d, self.s = heads, kv_heads, head_dim, seq
        self.scale, self.closed, self.use_hip = scale, closed, use_hip
        self.window = -1 if window < 0 or window >= seq - 1 else int(window)
        self.cos = to_device(cos.float().contiguous(), device)
        self.sin = to_device(sin.float().contiguous(), device)
        self.qk_norm = None
        if qk_norm is not None:
            qg, kg, eps = qk_norm
            self.qk_norm = (to_device(qg.float().reshape(-1).contiguous(), device),
                            to_device(kg.float().reshape(-1).contiguous(), device), float(eps))

    def __call__(self, ctx, node, ins):
        qkv = O.to_torch(ins[0])
        adder = O.to_torch(ins[1]) if len(ins) > 1 else None
        S, H, K, D = self.s, self.h, self.hkv, self.d
        W = (H + 2 * K) * D
        if qkv.numel() % (S * W):
            raise O.OpError(f"{node.name}: {list(qkv.shape)} is not [B * {S}, {W}]")
        B = qkv.numel() // (S * W)
        key_adder = adder is None or (adder.dim() == 4 and tuple(adder.shape[1:]) == (1, 1, S) and
                                      adder.shape[0] in (1, B))
        on_device = self.use_hip and qkv.is_cuda and H // K in ROPE_GROUPS and 1 <= S <= MAX_ATTENTION_SEQ and key_adder
        if on_device and D == 256:
            from ..ops import hip
            from .fused import _to_bf16
            q3 = _to_bf16(qkv).reshape(B, S, W).contiguous()
            ka = None if adder is None else adder.float().reshape(-1, S).contiguous().to(qkv.device)
            norm = self.qk_norm if self.qk_norm is not None else (None, None, 0.0)
            y = hip().rope_gqa_attention256(q3, self.cos, self.sin, ka, H, K, self.scale, self.window, None, *norm)
            return [y.reshape(B * S, H * D)]
        if on_device and D in ROPE_HEAD_DIMS and self.window < 0 and (self.qk_norm is None or D == 128):
            from ..ops import hip
            from .fused import _to_bf16
            q3 = _to_bf16(qkv).reshape(B, S, W).contiguous()
            ka = None if adder is None else adder.float().reshape(-1, S).contiguous().to(qkv.device)
            if self.qk_norm is None:
                y = hip().rope_gqa_attention(q3, self.cos, self.sin, ka, H, K, self.scale)
            else:
                y = hip().rope_gqa_attention(q3, self.cos, self.sin, ka, H, K, self.scale, None, *self.qk_norm)
            return [y.reshape(B * S, H * D)]
        f = qkv.float().reshape(B, S, W)
        cos = torch.cat([self.cos, self.cos], -1).to(f.device)
        sin = torch.cat([self.sin, self.sin], -1).to(f.device)

        def heads(t, n):              # [B, S, n * D] -> [B, H, S, D], each head repeated H / n times
            return t.reshape(B, S, n, 1, D).expand(B, S, n, H // n, D).reshape(B, S, H, D).permute(0, 2, 1, 3)

        def rot(t):
            return t * cos + torch.cat([-t[..., D // 2:], t[..., :D // 2]], -1) * sin

        def norm(t, gamma):
            if self.qk_norm is None:
                return t
            return t * torch.rsqrt((t * t).mean(-1, keepdim=True) + self.qk_norm[2]) * gamma.to(t.device)
        qg, kg = self.qk_norm[:2] if self.qk_norm is not None else (None, None)
        q, k = rot(norm(heads(f[..., :H * D], H), qg)), rot(norm(heads(f[..., H * D:(H + K) * D], K), kg))
        v = heads(f[..., (H + K) * D:], K)
        sc = q @ k.transpose(-1, -2) * self.scale
        band = torch.ones(S, S, dtype=torch.bool, device=sc.device).tril()
        if self.window >= 0:
            band = band & ~torch.ones(S, S, dtype=torch.bool, device=sc.device).tril(-self.window - 1)
        sc = torch.where(band, sc, torch.full_like(sc, self.closed))
        if adder is not None:
            sc = sc + adder.float().to(sc.device)
        y = (torch.softmax(sc, -1) @ v).permute(0, 2, 1, 3).reshape(B * S, H * D)
        return [y if not qkv.is_cuda else y.to(qkv.dtype)]


def fuse_rmsnorm(g, order, fed, fetch_refs, device, opts):
    """``Mul(Mul(x, Rsqrt(AddV2(Mean(Square(x), -1, keep_dims), eps))), gamma)`` (operands in
    either order, gamma a constant along the last axis) -> ``_RMSNorm(x)``.

    When x is an ``AddV2(a, b)`` of two non-constants that is not fetched and is
    read only by the norm and by at most one more node, itself an ``AddV2`` (the
    next residual add), the add goes in too: ``_RMSNorm(a, b)`` with the sum as
    output 1, which that reader takes.  An interior node read elsewhere, a Mean
    without keep_dims or over another axis, or a gamma that is not a row leaves
    the graph alone."""
    from .fused import _Ctx
    c = _Ctx(g, order, fed, fetch_refs, device, opts)
    for name in list(order):
        out = g.nodes.get(name)
        if out is None or out.op != "Mul" or len(out.inputs) != 2:
            continue
        for k in (0, 1):
            inner, gamma = _node(g, out.inputs[k]), _const_t(g, out.inputs[1 - k])
            if inner is not None and inner.op == "Mul" and len(inner.inputs) == 2 and gamma is not None:
                break
        else:
            continue
        gv = _last_axis_const(gamma)
        if gv is None or gv.numel() == 1 or not gv.is_floating_point():
            continue
        for k in (0, 1):
            rs, x_ref = _node(g, inner.inputs[k]), inner.inputs[1 - k]
            if rs is not None and rs.op == "Rsqrt":
                break
        else:
            continue
        add = _node(g, rs.inputs[0])
        if add is None or add.op not in ("Add", "AddV2") or len(add.inputs) != 2:
            continue
        for k in (0, 1):
            ms, eps = _node(g, add.inputs[k]), _scalar(g, add.inputs[1 - k])
            if ms is not None and ms.op == "Mean" and eps is not None:
                break
        else:
            continue
        sq = _node(g, ms.inputs[0])
        if not ms.attr("keep_dims", False) or not _axes_last(g, ms.inputs[1]) or sq is None or sq.op != "Square" or \
                sq.inputs[0] != x_ref:
            continue
        interior = [inner, rs, add, ms, sq]
        if not _interior_ok(c, interior, out):
            continue
        inputs = [x_ref]
        xs = _node(g, x_ref)
        if xs is not None and xs.op == "AddV2" and len(xs.inputs) == 2 and xs.name not in c.fetch_nodes and \
                all(_const_t(g, r) is None for r in xs.inputs):
            others = {cn for cn, _p, _i in c.cons.get(xs.name, [])} - {sq.name, inner.name}
            if len(others) <= 1 and all(g.nodes[cn].op == "AddV2" for cn in others):
                for cn in others:
                    g.nodes[cn].inputs = [(out.name, 1) if r == x_ref else r for r in g.nodes[cn].inputs]
                inputs = list(xs.inputs)
                interior.append(xs)
        _remove(g, interior)
        out.op = "_RMSNorm"
        out.inputs = inputs
        out.ctrl = []
        out.attrs = {"_impl": RMSNormOp(gv, eps, device, c.use_hip)}
        c.refresh()


def _rope_of(g, ref):
    """ref = AddV2(Mul(x, cos), Mul(ConcatV2(Neg(x2), x1, axis = -1), sin)) with x1, x2 = Split(x, 2, axis = -1)
    and cos, sin constants [S, D] under leading 1s whose two halves are equal
    -> (x ref, cos [S, D / 2], sin [S, D / 2], nodes), else None."""
    add = _node(g, ref)
    if add is None or add.op != "AddV2" or len(add.inputs) != 2:
        return None
    muls = [_node(g, r) for r in add.inputs]
    if any(m is None or m.op != "Mul" or len(m.inputs) != 2 for m in muls):
        return None

    def table(m):                    # Mul(t, const) in either order -> (t ref, const [S, D])
        for k in (0, 1):
            v = _const_t(g, m.inputs[k])
            if v is not None and v.dim() >= 2 and v.is_floating_point() and v.numel() == v.shape[-1] * v.shape[-2]:
                return m.inputs[1 - k], v.reshape(v.shape[-2], v.shape[-1])
        return None
    for mc, ms in (muls, muls[::-1]):
        tc, ts = table(mc), table(ms)
        cat = _node(g, ts[0]) if tc is not None and ts is not None else None
        if cat is None or cat.op != "ConcatV2" or len(cat.inputs) != 3 or _ints(g, cat.inputs[2]) != [-1]:
            continue
        x_ref, cos, sin = tc[0], tc[1], ts[1]
        neg, sp = _node(g, cat.inputs[0]), g.nodes.get(cat.inputs[1][0])
        if neg is None or neg.op != "Neg" or sp is None or sp.op != "Split" or int(sp.attr("num_split", 0)) != 2 or \
                cat.inputs[1] != (sp.name, 0) or neg.inputs[0] != (sp.name, 1) or sp.inputs[1] != x_ref or \
                _ints(g, sp.inputs[0]) != [-1]:
            continue
        half = cos.shape[1] // 2
        if cos.shape != sin.shape or cos.shape[1] % 2 or not torch.equal(cos[:, :half], cos[:, half:]) or \
                not torch.equal(sin[:, :half], sin[:, half:]):
            continue
        return x_ref, cos[:, :half], sin[:, :half], [add, mc, ms, cat, neg, sp]
    return None


def _group_heads_of(g, c, ref):
    """``_heads_of`` with, under the Reshape, an optional repeat of each head for its group:
    Reshape [-1, S, H, D] of Tile [1, 1, 1, G, 1] of Reshape [-1, S, H / G, 1, D]
    -> (dense ref, S, H, D, heads of the dense, nodes), else None."""
    h = _heads_of(g, c, ref)
    if h is None:
        return None
    src, S, H, D, nodes = h
    tile = _node(g, src)
    if tile is None or tile.op != "Tile":
        return src, S, H, D, H, nodes
    mult, r5 = _ints(g, tile.inputs[1]), _node(g, tile.inputs[0])
    shp = _ints(g, r5.inputs[1]) if r5 is not None and r5.op == "Reshape" else None
    if mult is None or len(mult) != 5 or shp is None or len(shp) != 5:
        return None
    G = mult[3]
    if mult != [1, 1, 1, G, 1] or G < 1 or H % G or shp != [-1, S, H // G, 1, D]:
        return None
    return r5.inputs[0], S, H, D, H // G, nodes + [tile, r5]


def _qk_norm_of(g, c, ref, S, n, D):
    """ref = _RMSNorm(Reshape(dense, [-1, S, n, D])) as fuse_rmsnorm made it, with one input (no
    residual), a gamma of D elements and output 1 unread -> (dense ref, gamma [D], eps, nodes), else None."""
    norm = _node(g, ref)
    if norm is None or norm.op != "_RMSNorm" or len(norm.inputs) != 1:
        return None
    impl = norm.attrs.get("_impl")
    r = _node(g, norm.inputs[0])
    if not isinstance(impl, RMSNormOp) or impl.g.numel() != D or r is None or r.op != "Reshape" or \
            _ints(g, r.inputs[1]) != [-1, S, n, D] or any(i != 0 for _cn, _p, i in c.cons.get(norm.name, [])):
        return None
    return r.inputs[0], impl.g.detach().cpu(), impl.eps, [norm, r]


def fuse_rope_attention(g, order, fed, fetch_refs, device, opts):
    """Llama's attention core -> _FusedQKV -> _RopeGQAttention: fuse_causal_attention's
    skeleton (``_causal_core``: the same masks, scale spellings and optional adder) with

    * q and k each rotated by position (``_rope_of``), with the same tables, of the pattern's S;
    * k and v each repeated for its group of query heads before the head transpose
      (``_group_heads_of``; no Tile when the group is one head), q not;
    * q, k, v from three denses on one input, H * D, Hkv * D and Hkv * D wide;
    * optionally (Qwen3's QK-norm) q and k each through ``_RMSNorm(Reshape(dense, [-1, S, n, D]))``
      before the repeat (``_qk_norm_of``): both or neither, with one eps, v never; the op then
      carries ``qk_norm``.  TFSERVE_QKNORM=0 (read at every compile) leaves such cores alone.
    * the mask either the triangle or (Gemma's local layers) a sliding window, the band {0 <= i - j <= w}
      for one w >= 0 in the same two spellings (``_window_mask``); the op then carries ``window`` = w.
      TFSERVE_GEMMA=0 (read at every compile) leaves windowed cores alone.

    Runs before fuse_causal_attention and takes nothing it takes: q and k must
    both be rotated.  A table whose halves differ, tables of another S or that
    differ between q and k, a rotated v, a Tile on another axis, or an interior
    node read elsewhere leaves the graph alone (fuse_causal_attention does not
    match it either: ``_heads_of`` finds an AddV2 or a Tile)."""
    from .fused import FusedMatMul, _Ctx
    c = _Ctx(g, order, fed, fetch_refs, device, opts)
    mask_of = _causal_mask if os.environ.get("TFSERVE_GEMMA", "1") == "0" else _window_mask
    for name in list(order):
        out = g.nodes.get(name)
        if out is None or out.op != "Reshape":
            continue
        core = _causal_core(g, out, mask_of)
        if core is None:
            continue
        qk, pv, S, scale, closed, adder_ref, interior, window = core
        rq, rk = _rope_of(g, qk.inputs[0]), _rope_of(g, qk.inputs[1])
        if rq is None or rk is None or not torch.equal(rq[1], rk[1]) or not torch.equal(rq[2], rk[2]):
            continue
        hq, hk, hv = _group_heads_of(g, c, rq[0]), _group_heads_of(g, c, rk[0]), _group_heads_of(g, c, pv.inputs[1])
        if hq is None or hk is None or hv is None or hq[1:4] != hk[1:4] or hq[1:4] != hv[1:4]:
            continue
        H, D, K = hq[2], hq[3], hk[4]
        if hq[1] != S or hq[4] != H or hv[4] != K or tuple(rq[1].shape) != (S, D // 2) or \
                _ints(g, out.inputs[1]) != [-1, H * D]:
            continue
        interior += rq[3] + rk[3] + hq[5] + hk[5] + hv[5]
        q_src, k_src, qk_norm = hq[0], hk[0], None
        nq, nk = _qk_norm_of(g, c, q_src, S, H, D), _qk_norm_of(g, c, k_src, S, K, D)
        if nq is not None and nk is not None and nq[2] == nk[2] and os.environ.get("TFSERVE_QKNORM", "1") != "0":
            q_src, k_src, qk_norm = nq[0], nk[0], (nq[1], nk[1], nq[2])
            interior += nq[3] + nk[3]
        if adder_ref is not None and adder_ref[0] in {n.name for n in interior}:
            continue
        dq, dk, dv = _dense_src(g, c, q_src), _dense_src(g, c, k_src), _dense_src(g, c, hv[0])
        if not (dq and dk and dv and dq[0] == dk[0] == dv[0]) or \
                [d[1].shape[1] for d in (dq, dk, dv)] != [H * D, K * D, K * D]:
            continue
        qkv_nodes = dq[3] + dk[3] + dv[3]
        if not _interior_ok(c, interior + qkv_nodes, out):
            continue
        qkv_name = g.unique_name(out.name + "/fused_qkv")
        w, b = torch.cat([dq[1], dk[1], dv[1]], dim=1), torch.cat([dq[2], dk[2], dv[2]])
        g.add(Node(name=qkv_name, op="_FusedQKV", inputs=[dq[0]],
                   attrs={"_impl": FusedMatMul(w, b, "none", False, device, c.use_hip, qkv_name)}))
        _remove(g, interior + qkv_nodes)
        out.op = "_RopeGQAttention"
        out.inputs = [(qkv_name, 0)] + ([adder_ref] if adder_ref is not None else [])
        out.ctrl = []
        out.attrs = {"_impl": RopeGQAttentionOp(H, K, D, S, scale, closed, rq[1], rq[2], device, c.use_hip, qk_norm,
                                                window)}
        c.refresh()


def fuse_swiglu(g, order, fed, fetch_refs, device, opts):
    """``Mul(_Swish(MatMul(x, Wg)), MatMul(x, Wu))`` (operands in either order; both
    denses bias-free, on one input, equally wide, read by nothing else) ->
    ``_FusedMatMul(x; [Wg | Wu])`` -> ``_SwiGLU``: x is read once.  Runs after
    fuse_swish, which spells the ``x * Sigmoid(x)``."""
    from .fused import FusedMatMul, _Ctx
    c = _Ctx(g, order, fed, fetch_refs, device, opts)
    for name in list(order):
        out = g.nodes.get(name)
        if out is None or out.op != "Mul" or len(out.inputs) != 2:
            continue
        for k in (0, 1):
            sw = _node(g, out.inputs[k])
            if sw is not None and sw.op == "_Swish":
                break
        else:
            continue
        dg, du = _dense_src(g, c, sw.inputs[0]), _dense_src(g, c, out.inputs[1 - k])
        if not (dg and du) or dg[0] != du[0] or len(dg[3]) != 1 or len(du[3]) != 1 or dg[1].shape != du[1].shape or \
                dg[3][0] is du[3][0]:
            continue
        interior = [sw] + dg[3] + du[3]
        if not _interior_ok(c, interior, out):
            continue
        mm_name = g.unique_name(out.name + "/gate_up")
        g.add(Node(name=mm_name, op="_FusedMatMul", inputs=[dg[0]],
                   attrs={"_impl": FusedMatMul(torch.cat([dg[1], du[1]], dim=1), None, "none", False, device,
                                               c.use_hip, mm_name)}))
        _remove(g, interior)
        out.op = "_SwiGLU"
        out.inputs = [(mm_name, 0)]
        out.ctrl = []
        out.attrs = {"_impl": SwiGLUOp(int(dg[1].shape[1]), c.use_hip)}
        c.refresh()


# ------------------------------------------------------------------ ModernBERT: RoPE encoder attention, GeGLU
class RopeAttentionOp:
    """Bidirectional attention over a packed [Q heads | K heads | V heads] buffer with q
    and k rotated by position (rotate-half, tables ``cos`` / ``sin`` [S, D / 2]).  Key j
    is open for query i iff ``|i - j| <= window``; ``window`` -1 opens every key.

    On the device, for D = 64, S within range and an adder that is absent or
    [B | 1, 1, 1, S], one ``rope_attention`` launch (kernels/rattn.hip): it rotates in
    fp32 and rounds to bf16 once, and closes the keys outside the window with -inf
    (docs/numerics.md, "RoPE encoder attention").  Anywhere else the graph's own
    arithmetic with torch, in fp32: the matched ``fill`` added outside the window."""

    def __init__(self, heads, head_dim, seq, scale, window, fill, cos, sin, device, use_hip):
        self.h, self.d, self.s = heads, head_dim, seq
        self.scale, self.window, self.fill, self.use_hip = scale, window, fill, use_hip
        self.cos = to_device(cos.float().contiguous(), device)
        self.sin = to_device(sin.float().contiguous(), device)

    def __call__(self, ctx, node, ins):
        qkv = O.to_torch(ins[0])
        adder = O.to_torch(ins[1]) if len(ins) > 1 else None
        S, H, D = self.s, self.h, self.d
        W = 3 * H * D
        if qkv.numel() % (S * W):
            raise O.OpError(f"{node.name}: {list(qkv.shape)} is not [B * {S}, {W}]")
        B = qkv.numel() // (S * W)
        key_adder = adder is None or (adder.dim() == 4 and tuple(adder.shape[1:]) == (1, 1, S) and
                                      adder.shape[0] in (1, B))
        if self.use_hip and qkv.is_cuda and D == 64 and 1 <= S <= MAX_ATTENTION_SEQ and key_adder:
            from ..ops import hip
            from .fused import _to_bf16
            q3 = _to_bf16(qkv).reshape(B, S, W).contiguous()
            ka = None if adder is None else adder.float().reshape(-1, S).contiguous().to(qkv.device)
            y = hip().rope_attention(q3, self.cos, self.sin, ka, H, self.scale, self.window)
            return [y.reshape(B * S, H * D)]
        f = qkv.float().reshape(B, S, 3, H, D).permute(2, 0, 3, 1, 4)
        cos = torch.cat([self.cos, self.cos], -1).to(f.device)
        sin = torch.cat([self.sin, self.sin], -1).to(f.device)

        def rot(t):
            return t * cos + torch.cat([-t[..., D // 2:], t[..., :D // 2]], -1) * sin
        sc = rot(f[0]) @ rot(f[1]).transpose(-1, -2) * self.scale
        if self.window >= 0:
            pos = torch.arange(S, device=sc.device)
            sc = sc + self.fill * ((pos[:, None] - pos[None, :]).abs() > self.window).float()
        if adder is not None:
            sc = sc + adder.float().to(sc.device)
        y = (torch.softmax(sc, -1) @ f[2]).permute(0, 2, 1, 3).reshape(B * S, H * D)
        return [y if not qkv.is_cuda else y.to(qkv.dtype)]


class GeGLUOp:
    """gelu_erf(gu[:, :F]) * gu[:, F:] after one GEMM over [W_gate | W_up]: ``geglu``
    (kernels/llama.hip) on the device for F % 8 == 0, else torch in fp32.  ``approximate``:
    the gate is the tanh form of the GELU (Gemma), the kernel's second build."""

    def __init__(self, width: int, use_hip: bool, approximate: bool = False):
        self.f, self.use_hip, self.approximate = width, use_hip, bool(approximate)

    def __call__(self, ctx, node, ins):
        gu = O.to_torch(ins[0])
        F_ = self.f
        if gu.shape[-1] != 2 * F_:
            raise O.OpError(f"{node.name}: {list(gu.shape)} is not [M, {2 * F_}]")
        if self.use_hip and gu.is_cuda and F_ % 8 == 0:
            from ..ops import hip
            from .fused import _to_bf16
            g2 = _to_bf16(gu).reshape(-1, 2 * F_).contiguous()
            y = hip().geglu(g2, None, True) if self.approximate else hip().geglu(g2)
            return [y.reshape(list(gu.shape[:-1]) + [F_])]
        gf = gu.float()
        y = F.gelu(gf[..., :F_], approximate="tanh" if self.approximate else "none") * gf[..., F_:]
        return [y if not gu.is_cuda else y.to(gu.dtype)]


def _reaches_qk(g, ref) -> bool:
    """Whether ref is q k^T (BatchMatMul, adj_y) under an optional scale and any number of adds."""
    n = _node(g, ref)
    if n is None:
        return False
    if n.op in ("Add", "AddV2") and len(n.inputs) == 2:
        return _reaches_qk(g, n.inputs[0]) or _reaches_qk(g, n.inputs[1])
    if n.op in ("Mul", "RealDiv"):
        sv = _scale_of(g, n)
        n = _node(g, sv[1]) if sv is not None else None
    return n is not None and n.op in _BMM and not n.attr("adj_x", False) and bool(n.attr("adj_y", False))


def _window_of(band: torch.Tensor, S: int):
    """band = fill * (|i - j| > w) as [S, S] under leading 1s, w >= 0 an integer and
    fill <= -MIN_CAUSAL_FILL -> (w, fill), else None.  w comes from row 0, then the whole matrix is compared.
    A band that closes nothing in row 0 (all zeros, or w >= S - 1) has no fill to read and is None too: such a
    graph stays unfused rather than being taken for the global form."""
    b = _square(band)
    if b is None or b.shape[0] != S or not b.is_floating_point():
        return None
    closed = torch.nonzero(b[0]).reshape(-1)
    if closed.numel() == 0 or int(closed[0]) == 0:
        return None                   # nothing closed in row 0: no fill to read; key 0 closed for query 0: no window
    w, fill = int(closed[0]) - 1, float(b[0, int(closed[0])])
    if not fill <= -MIN_CAUSAL_FILL:
        return None
    pos = torch.arange(S)
    want = torch.where((pos[:, None] - pos[None, :]).abs() > w, fill, 0.0).double()
    return (w, fill) if torch.equal(b.double().cpu(), want) else None


def fuse_rope_encoder_attention(g, order, fed, fetch_refs, device, opts):
    """ModernBERT's attention core -> _FusedQKV -> _RopeAttention: fuse_attention's skeleton::

        w = BatchMatMul(q, k, adj_y)  [Mul by c | RealDiv by c: _scale_of]
        scores = w [+ band] [+ adder]                     (AddV2, operands and the two adds in either order)
        y = Reshape(Transpose(BatchMatMul(Softmax(scores), v), [0, 2, 1, 3]), [-1, H * D])

    with q and k each rotated by position (``_rope_of``) with equal tables of the
    pattern's S and v not; q, k, v from three denses on one input, each H * D wide, or
    from one packed dense through Split / SplitV (``_split_qkv``); at most one
    non-constant ``adder`` (the op takes [B | 1, 1, 1, S] on the device) and at most
    one constant ``band``, which must be exactly ``fill * (|i - j| > w)`` (``_window_of``).
    window = w, or -1 without a band.

    Runs after fuse_rope_attention and takes nothing it takes: that pass needs a
    Sub or SelectV2 mask under the Softmax, this one only adds, and a causal band
    spelled as an adder is not symmetric.  A band with a hole, an asymmetric
    band, a weaker fill, a band that closes nothing in row 0, a per-head constant, tables that differ between q and k or are of
    another S, a rotated v, or an interior node read elsewhere leaves the graph
    alone."""
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
        # ---- the adds under the Softmax: at most one constant (the band) and one other (the adder)
        cur, band, adder_ref, ok = _node(g, sm.inputs[0]), None, None, True
        while ok and cur is not None and cur.op in ("Add", "AddV2") and len(cur.inputs) == 2:
            sides = [k for k in (0, 1) if _reaches_qk(g, cur.inputs[k])]
            if len(sides) != 1:
                ok = False
                break
            other = cur.inputs[1 - sides[0]]
            cv = _const_t(g, other)
            if cv is not None and band is None:
                band = cv
            elif cv is None and adder_ref is None:
                adder_ref = other
            else:
                ok = False
            interior.append(cur)
            cur = _node(g, cur.inputs[sides[0]])
        if not ok:
            continue
        scale = 1.0
        sv = _scale_of(g, cur) if cur is not None and cur.op in ("Mul", "RealDiv") else None
        if sv is not None:
            scale = sv[0]
            interior.append(cur)
            cur = _node(g, sv[1])
        qk = cur
        if qk is None or qk.op not in _BMM or qk.attr("adj_x", False) or not qk.attr("adj_y", False):
            continue
        interior.append(qk)
        rq, rk = _rope_of(g, qk.inputs[0]), _rope_of(g, qk.inputs[1])
        if rq is None or rk is None or not torch.equal(rq[1], rk[1]) or not torch.equal(rq[2], rk[2]):
            continue
        hq, hk, hv = _heads_of(g, c, rq[0]), _heads_of(g, c, rk[0]), _heads_of(g, c, pv.inputs[1])
        if hq is None or hk is None or hv is None or hq[1:4] != hk[1:4] or hq[1:4] != hv[1:4]:
            continue
        S, H, D = hq[1:4]
        if tuple(rq[1].shape) != (S, D // 2) or _ints(g, out.inputs[1]) != [-1, H * D]:
            continue
        window, fill = -1, 0.0
        if band is not None:
            wf = _window_of(band, S)
            if wf is None:
                continue
            window, fill = wf
        interior += rq[3] + rk[3] + hq[4] + hk[4] + hv[4]
        if adder_ref is not None and adder_ref[0] in {n.name for n in interior}:
            continue
        packed = _split_qkv(g, c, [hq[0], hk[0], hv[0]], H, D)
        if packed is not None:
            x_ref, w, b, qkv_nodes = packed
        else:
            dq, dk, dv = _dense_src(g, c, hq[0]), _dense_src(g, c, hk[0]), _dense_src(g, c, hv[0])
            if not (dq and dk and dv and dq[0] == dk[0] == dv[0]) or any(d[1].shape[1] != H * D for d in (dq, dk, dv)):
                continue
            x_ref = dq[0]
            w, b = torch.cat([dq[1], dk[1], dv[1]], dim=1), torch.cat([dq[2], dk[2], dv[2]])
            qkv_nodes = dq[3] + dk[3] + dv[3]
        if not _interior_ok(c, interior + qkv_nodes, out):
            continue
        qkv_name = g.unique_name(out.name + "/fused_qkv")
        g.add(Node(name=qkv_name, op="_FusedQKV", inputs=[x_ref],
                   attrs={"_impl": FusedMatMul(w, b, "none", False, device, c.use_hip, qkv_name)}))
        _remove(g, interior + qkv_nodes)
        out.op = "_RopeAttention"
        out.inputs = [(qkv_name, 0)] + ([adder_ref] if adder_ref is not None else [])
        out.ctrl = []
        out.attrs = {"_impl": RopeAttentionOp(H, D, S, scale, window, fill, rq[1], rq[2], device, c.use_hip)}
        c.refresh()


def fuse_geglu(g, order, fed, fetch_refs, device, opts):
    """``Mul(gelu_erf(s0), s1)`` (operands in either order) with ``s0, s1 = Split(dense(x), 2,
    axis = -1)`` of one bias-free dense read by nothing else -> ``_FusedMatMul(x; Wi)`` ->
    ``_GeGLU``.  The GELU is ``match_gelu_subgraph``'s erf form or its tanh form (Gemma;
    the op then carries ``approximate``); a biased dense, another axis or an interior node
    read elsewhere leaves the graph alone."""
    import types
    from .fused import FusedMatMul, _Ctx
    c = _Ctx(g, order, fed, fetch_refs, device, opts)
    for name in list(order):
        out = g.nodes.get(name)
        if out is None or out.op != "Mul" or len(out.inputs) != 2:
            continue
        for k in (0, 1):
            sp = g.nodes.get(out.inputs[k][0])
            if sp is not None and sp.op == "Split" and out.inputs[k] == (sp.name, 1) and len(sp.inputs) == 2 and \
                    int(sp.attr("num_split", 0)) == 2 and _ints(g, sp.inputs[0]) in ([-1], [1]):
                break
        else:
            continue
        ds = _dense_src(g, c, sp.inputs[1])
        if ds is None or len(ds[3]) != 1 or ds[1].shape[1] % 2:
            continue                  # (one MatMul node: no bias)
        # the GELU over output 0: the matcher wants every reader of the Split inside it, and ``out`` reads output 1
        readers = c.cons.get(sp.name, [])
        if [e for e in readers if e[2] == 1] != [(out.name, k, 1)]:
            continue
        view = types.SimpleNamespace(g=g, fetch_nodes=c.fetch_nodes,
                                     cons={**c.cons, sp.name: [e for e in readers if e[2] == 0]})
        m = match_gelu_subgraph(g, view, sp.name)
        if m is None or m[0] not in ("gelu_erf", "gelu_tanh") or (m[2].name, 0) != out.inputs[1 - k]:
            continue
        interior = m[1] + [m[2], sp] + ds[3]
        if not _interior_ok(c, interior, out):
            continue
        mm_name = g.unique_name(out.name + "/gate_up")
        g.add(Node(name=mm_name, op="_FusedMatMul", inputs=[ds[0]],
                   attrs={"_impl": FusedMatMul(ds[1], None, "none", False, device, c.use_hip, mm_name)}))
        _remove(g, interior)
        out.op = "_GeGLU"
        out.inputs = [(mm_name, 0)]
        out.ctrl = []
        out.attrs = {"_impl": GeGLUOp(int(ds[1].shape[1]) // 2, c.use_hip, m[0] == "gelu_tanh")}
        c.refresh()


# ------------------------------------------------------------------ T5: attention with a relative-position bias
class BiasAttentionOp:
    """Bidirectional attention over a packed [Q heads | K heads | V heads] buffer with a
    per-head bias that depends on j - i only: ``table`` [H, 2 S - 1], entry j - i + S - 1
    (T5's relative-position bias; any exactly Toeplitz [H, S, S] constant).  Inputs
    ``[qkv, adder?]``.

    On the device, for D = 64, S within range and an adder that is absent or
    [B | 1, 1, 1, S], one ``bias_attention`` launch (kernels/battn.hip; docs/numerics.md,
    "Relative-bias attention").  Anywhere else the graph's own arithmetic with torch, in
    fp32: the dense [H, S, S] bias rebuilt from the table by indexing, which is the
    matched constant bit for bit, added to the scores before the adder, or summed with
    the adder first (``sum_first``) where the graph shares that sum between its layers."""

    def __init__(self, heads, head_dim, seq, scale, table, device, use_hip, sum_first=False):
        self.h, self.d, self.s = heads, head_dim, seq
        self.scale, self.use_hip, self.sum_first = scale, use_hip, bool(sum_first)
        self.table = to_device(table.float().contiguous(), device)

    def dense_bias(self, device) -> torch.Tensor:
        """[1, H, S, S] f32: table[h, j - i + S - 1]."""
        pos = torch.arange(self.s, device=device)
        return self.table.to(device)[:, pos[None, :] - pos[:, None] + (self.s - 1)][None]

    def __call__(self, ctx, node, ins):
        qkv = O.to_torch(ins[0])
        adder = O.to_torch(ins[1]) if len(ins) > 1 else None
        S, H, D = self.s, self.h, self.d
        W = 3 * H * D
        if qkv.numel() % (S * W):
            raise O.OpError(f"{node.name}: {list(qkv.shape)} is not [B * {S}, {W}]")
        B = qkv.numel() // (S * W)
        key_adder = adder is None or (adder.dim() == 4 and tuple(adder.shape[1:]) == (1, 1, S) and
                                      adder.shape[0] in (1, B))
        if self.use_hip and qkv.is_cuda and D == 64 and 1 <= S <= MAX_ATTENTION_SEQ and key_adder:
            from ..ops import hip
            from .fused import _to_bf16
            q3 = _to_bf16(qkv).reshape(B, S, W).contiguous()
            ka = None if adder is None else adder.float().reshape(-1, S).contiguous().to(qkv.device)
            y = hip().bias_attention(q3, self.table, ka, H, self.scale)
            return [y.reshape(B * S, H * D)]
        q, k, v = qkv.float().reshape(B, S, 3, H, D).permute(2, 0, 3, 1, 4)
        sc = q @ k.transpose(-1, -2)
        if self.scale != 1.0:
            sc = sc * self.scale
        bias = self.dense_bias(sc.device)
        if adder is None:
            sc = sc + bias
        elif self.sum_first:
            sc = sc + (bias + adder.float().to(sc.device))
        else:
            sc = sc + bias + adder.float().to(sc.device)
        y = (torch.softmax(sc, -1) @ v).permute(0, 2, 1, 3).reshape(B * S, H * D)
        return [y if not qkv.is_cuda else y.to(qkv.dtype)]


def _head_bias_shaped(v: torch.Tensor) -> bool:
    """[1, H, S, S] or [H, S, S], by shape."""
    return v.is_floating_point() and v.dim() in (3, 4) and v.shape[-1] == v.shape[-2] and (v.dim() == 3 or v.shape[0] == 1)


def _toeplitz_table(bias: torch.Tensor, H: int, S: int) -> Optional[torch.Tensor]:
    """bias [1, H, S, S] | [H, S, S] with b[h, i, j] == b[h, i + 1, j + 1] everywhere (compared for
    equality) -> its diagonals [H, 2 S - 1], entry j - i + S - 1, else None.  Indexing only: a meta
    constant (a replica that receives its weights) gives a meta table and is taken on its shape, the
    values having been compared where the weights were read."""
    if not _head_bias_shaped(bias):
        return None
    b = bias[0] if bias.dim() == 4 else bias
    if tuple(b.shape) != (H, S, S):
        return None
    if not b.is_meta and not torch.equal(b[:, :-1, :-1], b[:, 1:, 1:]):
        return None
    return torch.cat([b[:, 1:, 0].flip(-1), b[:, 0, :]], -1)


def fuse_bias_attention(g, order, fed, fetch_refs, device, opts):
    """T5's attention core -> _FusedQKV -> _BiasAttention: fuse_attention's skeleton::

        w = BatchMatMul(q, k, adj_y)  [Mul by c | RealDiv by c: _scale_of; T5 has none]
        scores = (w + bias) + adder   |   w + (bias + adder)          (AddV2, operands in either order)
        y = Reshape(Transpose(BatchMatMul(Softmax(scores), v), [0, 2, 1, 3]), [-1, H * D])

    with exactly one constant ``bias`` shaped [1, H, S, S] or [H, S, S] that is exactly
    Toeplitz per head (``_toeplitz_table``) and at most one non-constant ``adder`` (the op
    takes [B | 1, 1, 1, S] on the device); q, k, v from three denses on one input, with a
    bias or without.  In the second spelling ``bias + adder`` is computed once and read by
    every layer: that node is not interior, it is bypassed (the op reads ``adder``) and
    stays until its last reader is rewritten, after which nothing reaches it.

    Runs directly before fuse_attention.  No earlier pass takes a core with a constant
    per-head bias (fuse_window_attention needs the window reshapes around it), and what
    this pass leaves -- a bias that is not Toeplitz, two constants, a per-head constant of
    another S or H, a per-head bias that is not constant, an interior node read elsewhere
    -- fuse_attention sees unchanged."""
    from .fused import FusedMatMul, _Ctx
    c = _Ctx(g, order, fed, fetch_refs, device, opts)
    tables = {}                       # bias Const ref -> table | None: the layers share one constant
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
        # ---- the adds under the Softmax: one constant (the bias) and at most one other (the adder)
        cur, biases, adders, ok, sum_first = _node(g, sm.inputs[0]), [], [], True, False
        while cur is not None and cur.op in ("Add", "AddV2") and len(cur.inputs) == 2:
            sides = [k for k in (0, 1) if _reaches_qk(g, cur.inputs[k])]
            if len(sides) != 1:
                ok = False
                break
            other = cur.inputs[1 - sides[0]]
            if _const_t(g, other) is not None:
                biases.append(other)
            else:
                shared = _node(g, other)          # bias + adder, shared by the layers?
                parts = None
                if shared is not None and shared.op in ("Add", "AddV2") and len(shared.inputs) == 2:
                    for k in (0, 1):
                        cv = _const_t(g, shared.inputs[k])
                        if cv is not None and _head_bias_shaped(cv) and _const_t(g, shared.inputs[1 - k]) is None:
                            parts = (shared.inputs[k], shared.inputs[1 - k])
                if parts is not None:
                    biases.append(parts[0])
                    adders.append(parts[1])
                    sum_first = True
                else:
                    adders.append(other)
            interior.append(cur)
            cur = _node(g, cur.inputs[sides[0]])
        if not ok or len(biases) != 1 or len(adders) > 1:
            continue
        adder_ref = adders[0] if adders else None
        scale = 1.0
        sv = _scale_of(g, cur) if cur is not None and cur.op in ("Mul", "RealDiv") else None
        if sv is not None:
            scale = sv[0]
            interior.append(cur)
            cur = _node(g, sv[1])
        qk = cur
        if qk is None or qk.op not in _BMM or qk.attr("adj_x", False) or not qk.attr("adj_y", False):
            continue
        interior.append(qk)
        hq, hk, hv = _heads_of(g, c, qk.inputs[0]), _heads_of(g, c, qk.inputs[1]), _heads_of(g, c, pv.inputs[1])
        if hq is None or hk is None or hv is None or hq[1:4] != hk[1:4] or hq[1:4] != hv[1:4]:
            continue
        S, H, D = hq[1:4]
        fshape = _ints(g, out.inputs[1])
        if fshape is None or len(fshape) != 2 or fshape[-1] != H * D:
            continue                  # (the op returns [B * S, H * D])
        if biases[0] not in tables:
            tables[biases[0]] = _toeplitz_table(_const_t(g, biases[0]), H, S)
        table = tables[biases[0]]
        if table is None or tuple(table.shape) != (H, 2 * S - 1):
            continue
        interior += hq[4] + hk[4] + hv[4]
        if adder_ref is not None and adder_ref[0] in {n.name for n in interior}:
            continue
        dq, dk, dv = _dense_src(g, c, hq[0]), _dense_src(g, c, hk[0]), _dense_src(g, c, hv[0])
        if not (dq and dk and dv and dq[0] == dk[0] == dv[0]) or any(d[1].shape[1] != H * D for d in (dq, dk, dv)):
            continue
        qkv_nodes = dq[3] + dk[3] + dv[3]
        if not _interior_ok(c, interior + qkv_nodes, out):
            continue
        w, b = torch.cat([dq[1], dk[1], dv[1]], dim=1), torch.cat([dq[2], dk[2], dv[2]])
        qkv_name = g.unique_name(out.name + "/fused_qkv")
        g.add(Node(name=qkv_name, op="_FusedQKV", inputs=[dq[0]],
                   attrs={"_impl": FusedMatMul(w, b, "none", False, device, c.use_hip, qkv_name)}))
        _remove(g, interior + qkv_nodes)
        out.op = "_BiasAttention"
        out.inputs = [(qkv_name, 0)] + ([adder_ref] if adder_ref is not None else [])
        out.ctrl = []
        out.attrs = {"_impl": BiasAttentionOp(H, D, S, scale, table, device, c.use_hip, sum_first)}
        c.refresh()


def t5_passes():
    """TFSERVE_T5=0 (read at every compile) removes the pass: the engine A/B in one build."""
    return [] if os.environ.get("TFSERVE_T5", "1") == "0" else [fuse_bias_attention]


def modernbert_passes():
    """TFSERVE_MODERNBERT=0 (read at every compile) removes the two passes: the engine A/B in one build."""
    return [] if os.environ.get("TFSERVE_MODERNBERT", "1") == "0" else [fuse_rope_encoder_attention, fuse_geglu]


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
    return [fuse_layernorm, fuse_rmsnorm, fuse_embedding, fuse_window_attention, fold_window_layout, fuse_rope_attention,
            fuse_causal_attention] + t5_passes() + [fuse_attention, fuse_key_mask, fuse_swiglu] + modernbert_passes()


def late_passes():
    """Passes over the fused graph (after every GEMM is a _FusedMatMul).  None
    here; the LayerNorm fold runs last (graph/fused.py defer_layernorm: round
    3's fold spilled registers in the 8-wave tiles and was removed in round 4,
    profiles/round3/ln_fold.md; round 5's epilogue reads its per-column
    vectors from LDS instead)."""
    return []
