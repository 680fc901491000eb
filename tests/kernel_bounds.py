"""fp64 references and elementwise error bounds for the HIP kernels.

A plain helper module (no fixtures, nothing at collection time).  Every
reference takes the bf16-rounded operands upcast exactly to fp64; every bound
is derived from what the kernel does (docs/numerics.md has the derivations in
prose) and holds for EVERY output element:

    |y - ref| <= bound            (assert_within; no element is left out)

Error model
-----------
U_BF16 = 2^-8   one round-to-nearest-even store to bf16 (8 significant bits:
                half an ulp is at most 2^-8 |x|; a truncating store is wrong
                by up to 2^-7 |x| and must fail),
U_F32  = 2^-24  one rounding to fp32,
E      = 2^-23  per fp32 operation.  Twice the rounding unit, so it also covers
                MFMA accumulation that is not strictly round-to-nearest.

A constant here changes only by re-deriving it from the kernel's code, with the
derivation in the comment -- never by scaling it until a failing kernel passes.
"""
import math

import torch
import torch.nn.functional as F

U_BF16 = 2.0 ** -8
U_F32 = 2.0 ** -24
E = 2.0 ** -23

BF = torch.bfloat16


def rnd(*shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def d(t):
    """Exact upcast to fp64 (None stays None)."""
    return None if t is None else t.detach().cpu().double()


def u_out(out_f32):
    return U_F32 if out_f32 else U_BF16


# ---------------------------------------------------------------- the checker
def assert_within(y, ref, bound, what=""):
    """Every element: |y - ref| <= bound.  Returns the worst err / bound.

    A non-finite y (or one whose error is NaN) fails; where err == 0 the ratio
    is 0 even if the bound is 0 (exact cases)."""
    y = d(y)
    ref = d(ref)
    bound = d(bound).expand_as(ref) if torch.is_tensor(bound) else torch.full_like(ref, float(bound))
    assert y.shape == ref.shape, f"{what}: shape {tuple(y.shape)} != {tuple(ref.shape)}"
    assert torch.isfinite(ref).all() and torch.isfinite(bound).all(), f"{what}: non-finite reference / bound"
    err = (y - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    ratio = torch.where(torch.isfinite(y) & ~torch.isnan(ratio), ratio, torch.full_like(ratio, float("inf")))
    worst = ratio.max().item() if ratio.numel() else 0.0
    if worst > 1.0:
        bad = ratio > 1.0
        i = int(ratio.argmax())
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ratio.shape))
        raise AssertionError(
            f"{what}: {int(bad.sum())} of {ratio.numel()} elements outside the bound; worst err/bound = "
            f"{worst:.3f} at {idx}: y = {y.flatten()[i].item():.9g}, ref = {ref.flatten()[i].item():.9g}, "
            f"bound = {bound.flatten()[i].item():.3g}")
    return worst


# ---------------------------------------------------------------- activations
def act64(act, x):
    if act == "relu":
        return torch.relu(x)
    if act == "gelu_tanh":
        return F.gelu(x, approximate="tanh")
    if act == "gelu_erf":
        return F.gelu(x)
    if act == "tanh":
        return torch.tanh(x)
    assert act == "none", act
    return x


# Lipschitz constants: |relu'|, |tanh'| <= 1; GELU' peaks at 1.129 (x ~ 1.41).
L_ACT = {"none": 1.0, "relu": 1.0, "tanh": 1.0, "gelu_tanh": 1.13, "gelu_erf": 1.13}

# Absolute error of the activation itself, c * E * (1 + |pre|), from the <= 1 ulp
# (= E relative) accuracy of v_exp_f32 / v_rcp_f32 that common.h relies on:
#
#  sigm2(u) = rcp(1 + exp(-2u)).  t = exp(-2u) is exp2 of the rounded product
#    -2u * log2(e): the product and the constant contribute 1.5 E relative to
#    the argument, i.e. 1.5 E * 2|u| relative to t, plus 1 ulp of v_exp:
#    dt/t <= (1 + 3|u|) E.  s = 1/(1 + t): ds/s <= t/(1+t) * dt/t + 2 E (the add,
#    the rcp).  |u| t/(1+t) <= 0.19 for u > 0 and s |u| <= 0.19 for u < 0
#    (max of u exp(-2u)), so ds <= (1 + 0.6 + 2) E < 4 E absolute.
#  tanh = 2 s - 1: 2 ds + one rounding of a value <= 1  ->  9 E.         c = 9
#  gelu_tanh = x * rcp(1 + exp2(x t)), t = fma(x^2, k1, k0): the argument
#    carries 4 roundings + two constants (<= 5 E relative; |arg| = 2|u| log2 e
#    with u = sqrt(2/pi)(x + 0.044715 x^3)), so dt/t <= (1 + 10|u|) E and
#    |x| ds <= |x| s (1 + 2) E + 10 E |x||u| t/(1+t)^2.  |u| >= 0.79 |x| and
#    t/(1+t)^2 <= exp(-2|u|) give |x||u| exp(-2|u|) <= 1.27 max(v^2 exp(-2v))
#    = 0.172, so the last term is <= 1.8 E; with the final product's rounding
#    the total is <= (1.8 + 4 |x|) E.                                   c = 4
#  gelu_erf = 0.5 x (1 + erff(x / sqrt 2)): erff is documented at 4 ulp (HIP
#    math API), the argument's rounding adds 1.5 E |a| erf'(a) <= 0.7 E, the
#    add 2 E (|1 + erf| <= 2), two more products: 0.5 |x| (4 + 0.7 + 2) E + 2 E
#    |gelu| <= 5.4 E |x|.                                                c = 6
C_ACT = {"none": 0.0, "relu": 0.0, "tanh": 9.0, "gelu_tanh": 4.0, "gelu_erf": 6.0}


def act_abs(act, pre):
    return C_ACT[act] * E * (1.0 + pre.abs())


# ---------------------------------------------------------------- GEMM / conv
def gemm_parts(x, w, bias=None, res=None):
    """x [M, K], w [N, K] (bf16-valued) -> (pre, mag) in fp64:
    pre = x w^T + bias + res, mag = |x| |w|^T + |bias| + |res|."""
    x, w = d(x), d(w)
    pre = x @ w.t()
    mag = x.abs() @ w.abs().t()
    if bias is not None:
        pre = pre + d(bias)
        mag = mag + d(bias).abs()
    if res is not None:
        pre = pre + d(res)
        mag = mag + d(res).abs()
    return pre, mag


def conv_parts(x, w_hwio, bias=None, stride=1, pads=(0, 0, 0, 0), res=None):
    """NHWC x, HWIO w, pads (top, bottom, left, right) -> (pre, mag), NHWC fp64."""
    pt, pb, pl, pr = pads
    sh, sw = (stride, stride) if isinstance(stride, int) else stride
    x, w = d(x), d(w_hwio)

    def conv(xx, ww):
        return F.conv2d(F.pad(xx.permute(0, 3, 1, 2), [pl, pr, pt, pb]), ww.permute(3, 2, 0, 1),
                        stride=(sh, sw)).permute(0, 2, 3, 1)
    pre, mag = conv(x, w), conv(x.abs(), w.abs())
    if bias is not None:
        pre = pre + d(bias)
        mag = mag + d(bias).abs()
    if res is not None:
        pre = pre + d(res)
        mag = mag + d(res).abs()
    return pre, mag


def acc_bound(pre, mag, k, splits, act):
    """fp32 error of act(pre) before the output rounding.

    A K-deep dot product accumulated in fp32 in any order is off by at most
    K E sum|a_i b_i|; each split-K slab adds one more addition, and bias,
    residual, the activation's own products add at most 4 more operations:
        (K + splits + 4) E (|A| |B| + |bias| + |res|),
    pushed through the activation (Lipschitz L_act) plus its own error."""
    return L_ACT[act] * (k + splits + 4) * E * mag + act_abs(act, pre)


def out_bound(ref, acc, out_f32):
    """One rounding of the (slightly wrong) fp32 value to the output type."""
    u = u_out(out_f32)
    return u * (ref.abs() + acc) + acc


def epilogue(pre, mag, k, splits=1, act="none", out_f32=False):
    """(ref, bound) of a GEMM / conv epilogue."""
    ref = act64(act, pre)
    return ref, out_bound(ref, acc_bound(pre, mag, k, splits, act), out_f32)


def post_output(pre, mag, k, splits, scale, shift, act2="relu", out_f32=False):
    """The second output of a conv: act2(v * scale + shift) per channel.

    gemm_common.h post_chunk applies the affine to the fp32 epilogue value v
    (not to the rounded first output), so no bf16 term propagates: v's error
    is scaled by |scale| and the multiply-add adds two roundings."""
    scale, shift = d(scale), d(shift)
    pre2 = pre * scale + shift
    acc = acc_bound(pre, mag, k, splits, "none") * scale.abs() + 2 * E * ((pre * scale).abs() + shift.abs())
    ref2 = act64(act2, pre2)
    return ref2, out_bound(ref2, L_ACT[act2] * acc + act_abs(act2, pre2), out_f32)


def propagated(intermediate, w):
    """Error an unseen bf16-rounded intermediate [M, K] carries into the next
    GEMM with w [N, K]: 2^-8 |intermediate| |W|^T."""
    return U_BF16 * (d(intermediate).abs() @ d(w).abs().t())


# ---------------------------------------------------------------- LayerNorm
def layernorm_ref(z, gamma, beta, eps, dz=None, out_f32=False):
    """(ref, bound) of LN(z) * gamma + beta over the last axis, z in fp64.

    The kernels keep the row in fp32, take the mean and the (biased, two-pass)
    variance over `cols` terms, then xhat * gamma + beta and one bf16 store:
        dxh  = (cols + 8) E (mean|z| rstd + |xhat|) + 8 E |xhat|
        acc  = dxh |gamma| + 2 E |xhat gamma| + E |ref|
        bound = u_out (|ref| + acc) + acc
    dz: elementwise error already in z (a GEMM's accumulation in linear_ln).
    To first order d xhat_i = (dz_i - d mu) rstd - xhat_i d sigma rstd with
    |d mu| <= mean dz and |d sigma| <= max dz + mean dz, which adds
        rstd (dz_i + mean dz + |xhat_i| (max dz + mean dz))."""
    z, gamma, beta = d(z), d(gamma), d(beta)
    cols = z.shape[-1]
    mu = z.mean(-1, keepdim=True)
    var = ((z - mu) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    xhat = (z - mu) * rstd
    ref = xhat * gamma + beta
    dxh = (cols + 8) * E * (z.abs().mean(-1, keepdim=True) * rstd + xhat.abs()) + 8 * E * xhat.abs()
    if dz is not None:
        dz = d(dz)
        mdz, xdz = dz.mean(-1, keepdim=True), dz.amax(-1, keepdim=True)
        dxh = dxh + rstd * (dz + mdz + xhat.abs() * (xdz + mdz))
    acc = dxh * gamma.abs() + 2 * E * (xhat * gamma).abs() + E * ref.abs()
    return ref, out_bound(ref, acc, out_f32)


def row_partials(t, parts):
    """[M][parts][2] fp32 (sum, sum sq) over `parts` column slices of t's rows:
    what a deferred-LayerNorm producer hands on, here summed in fp64 and
    rounded once, so the statistics the kernel is given are off by 2^-24."""
    f = d(t)
    cols = torch.tensor_split(torch.arange(f.shape[1]), parts)
    return torch.stack([torch.stack([f[:, c].sum(1), (f[:, c] ** 2).sum(1)], 1) for c in cols], 1).float().contiguous()


def ln_stats_err(z, parts, eps):
    """Exact (mean, rstd) of z's rows and the error of the kernels' one-pass
    statistics from `parts` fp32 partials (gemm_common.h ln_row_stats):
        mean = (sum of the partial sums) / len          d mean <= (parts + 3) E mean|z|
        var  = (sum of the partial squares) / len - mean^2
                                                         d var  <= (parts + 6) E (E[z^2] + mean^2) + 2 |mean| d mean
        rstd = rsqrt(max(var, 0) + eps)                  d rstd / rstd <= d var / (2 (var + eps)) + 3 E
    (the E[z^2] - mean^2 cancellation is in d var / var: the bound widens by
    itself for rows whose mean dwarfs their spread)."""
    mean = z.mean(-1, keepdim=True)
    msq = (z * z).mean(-1, keepdim=True)
    var = ((z - mean) ** 2).mean(-1, keepdim=True)
    dmean = (parts + 3) * E * z.abs().mean(-1, keepdim=True)
    dvar = (parts + 6) * E * (msq + mean ** 2) + 2 * mean.abs() * dmean
    return mean, 1.0 / torch.sqrt(var + eps), dmean, dvar / (2 * (var + eps)) + 3 * E


def lnx_ref(x, w, bias, act, a_parts=0, a_eps=0.0, colsum=None, zr=None, r_parts=0, r_gamma=None, r_beta=None,
            r_eps=0.0, out_f32=False):
    """(ref, bound) of the deferred-LayerNorm GEMM (cgemm_impl.h epilogue_lnx):

        y = act( rstd_a (x w^T - mean_a colsum) + bias + (zr - mean_r) rstd_r gamma + beta )

    with x's (a_parts > 0) and / or the residual's (r_parts > 0) LayerNorm
    applied from row statistics.  The reference centres exactly,
    rstd_a ((x - mean_a) w^T), so it has no cancellation of its own; the
    kernel's x w^T - mean colsum does, and the bound says by how much:
        dD = (K + 2) E |x| |w|^T + (d mean + (2^-24 + 2 E) |mean|) |colsum|
    (fp32 accumulation; the mean's error, the rounding of the colsum it is
    given -- summed in fp64 and rounded once -- and the product and the
    subtraction), dT = rstd dD + (d rstd / rstd + 3 E) |T|.  The residual
    side is elementwise: dR = rstd_r |gamma| (d mean_r + E |zr - mean_r|)
    + (d rstd_r / rstd_r + 3 E) |xhat gamma| + E |beta|.  Four more fp32
    operations join T, bias and R; then the activation and one store."""
    x64, w64 = d(x), d(w)[:, :x.shape[1]]
    k = x64.shape[1]
    if a_parts:
        mean, rstd, dmean, rel = ln_stats_err(x64, a_parts, a_eps)
        t = rstd * ((x64 - mean) @ w64.t())
        dd = (k + 2) * E * (x64.abs() @ w64.abs().t()) + (dmean + (U_F32 + 2 * E) * mean.abs()) * d(colsum).abs()
        dt = rstd * dd + (rel + 3 * E) * t.abs()
    else:
        t = x64 @ w64.t()
        dt = (k + 2) * E * (x64.abs() @ w64.abs().t())
    pre, err, mag = t, dt, t.abs()
    if bias is not None:
        pre = pre + d(bias)
        mag = mag + d(bias).abs()
    if zr is not None:
        z = d(zr)
        if r_parts:
            mean, rstd, dmean, rel = ln_stats_err(z, r_parts, r_eps)
            g, b = d(r_gamma), d(r_beta)
            xg = (z - mean) * rstd * g
            r = xg + b
            err = err + rstd * g.abs() * (dmean + E * (z - mean).abs()) + (rel + 3 * E) * xg.abs() + E * b.abs()
        else:
            r = z
        pre = pre + r
        mag = mag + r.abs()
    err = err + 4 * E * mag
    ref = act64(act, pre)
    return ref, out_bound(ref, L_ACT[act] * err + act_abs(act, pre), out_f32)


def stats_bound(y, n_tiles):
    """The (sum, sum sq) a deferred-LayerNorm GEMM emits for its stored bf16
    rows y [M, N]: N additions in any order (LDS atomics) in `n_tiles` column
    tiles summed by the reader -> (exact sums [M, 2], bounds [M, 2])."""
    y = d(y)
    n = y.shape[1]
    sums = torch.stack([y.sum(1), (y * y).sum(1)], 1)
    return sums, (n + n_tiles + 4) * E * torch.stack([y.abs().sum(1), (y * y).sum(1)], 1)


def embed_sum(ids, type_ids, word, pos, typ, seq):
    """fp64 word + position + type rows; ids outside a table add a zero row."""
    word = d(word)
    ids = ids.reshape(-1).long()
    ok = (ids >= 0) & (ids < word.shape[0])
    z = torch.where(ok[:, None], word[ids.clamp(0, word.shape[0] - 1)], torch.zeros((), dtype=torch.float64))
    if pos is not None:
        z = z + d(pos)[torch.arange(ids.numel()) % seq]
    if type_ids is not None:
        typ = d(typ)
        tt = type_ids.reshape(-1).long()
        okt = (tt >= 0) & (tt < typ.shape[0])
        z = z + torch.where(okt[:, None], typ[tt.clamp(0, typ.shape[0] - 1)], torch.zeros((), dtype=torch.float64))
    return z


# ---------------------------------------------------------------- attention
def attention_ref(qkv, heads, scale, mask=None):
    """qkv [B, S, 3 H D] bf16-valued, mask None / [B, S] / [B, 1, S, S] adder
    -> (ref, bound) [B, S, H D].

    The kernels compute s = (q . k) scale + mask in fp32, p = exp(s - max),
    round p to bf16 for the P V MFMA, sum the unrounded p in fp32, accumulate
    P V in fp32, divide and store bf16.  Per key j the numerator p_j v_j is
    off by (2^-8 [P to bf16] + ds_j [score]) relatively, the denominator by
    sum_j p_j ds_j, and the two S-term fp32 sums, the exp and the divide
    together by (S + 16) E (E is twice the rounding unit, S/2 E per sum):

        bound = ( sum_j p_j |v_j| (2^-8 + ds_j) + (P |V|) (sum_j p_j ds_j + (S + 16) E) ) (1 + 2^-8)
                + 2^-8 |ref|
        ds_j  = (D + 4) E (|q| . |k_j|) scale + E |s_j|

    This weights each key's score error by its probability; it is never
    larger than taking max_j ds_j over the row (rel = 2^-8 + 2 ds + (S+16) E),
    and keys with p_j == 0 (masked by -10000, the fp32 minimum or -inf)
    contribute nothing, whatever rounding their huge |s_j| suffers."""
    b, s, hd3 = qkv.shape
    dh = hd3 // (3 * heads)
    q, k, v = d(qkv).reshape(b, s, 3, heads, dh).permute(2, 0, 3, 1, 4)
    sc = q @ k.transpose(-1, -2) * scale
    asc = q.abs() @ k.abs().transpose(-1, -2) * scale
    if mask is not None:
        m = d(mask)
        sc = sc + (m[:, None, None, :] if m.dim() == 2 else m)
    p = torch.softmax(sc, -1)
    assert torch.isfinite(p).all(), "a query row with no open key has no defined result"
    ds = (dh + 4) * E * asc + E * sc.abs()
    ds = torch.where(p > 0, ds, torch.zeros_like(ds))
    pav = p @ v.abs()
    ref = p @ v
    num = (p * (U_BF16 + ds)) @ v.abs()
    den = (p * ds).sum(-1, keepdim=True) + (s + 16) * E
    bound = (num + pav * den) * (1 + U_BF16) + U_BF16 * ref.abs()

    def merge(t):
        return t.permute(0, 2, 1, 3).reshape(b, s, heads * dh)
    return merge(ref), merge(bound)


# ---------------------------------------------------------------- pools, softmax
def gap_ref(x):
    """NHWC -> (mean over H W, bound): HW fp32 additions, the 1/HW product and
    one more operation, then one bf16 store:
        u_out |ref| + (HW + 2) E mean|x|   (+ the u_out of that small term)."""
    x = d(x)
    hw = x.shape[1] * x.shape[2]
    ref = x.mean((1, 2))
    acc = (hw + 2) * E * x.abs().mean((1, 2))
    return ref, out_bound(ref, acc, False), acc


def softmax_ref(logits, dlogit=None):
    """(probs, bound) of an fp32 softmax over the last axis.

    p_i = exp(l_i - max) / sum: `cols` additions, the exp (argument rounding
    times |l_i - max| p_i <= p_i e^-1-ish, 1 ulp), the reciprocal and the
    product are covered by (cols + 16) E p_i.  A logit error dl_j moves p_i by
    p_i (dl_i + sum_j p_j dl_j) <= 2 max(dl) p_i; the fp32 store adds 2^-24 p."""
    lg = d(logits)
    p = torch.softmax(lg, -1)
    cols = lg.shape[-1]
    bound = (cols + 16) * E * p + U_F32 * p
    if dlogit is not None:
        dl = d(dlogit) if torch.is_tensor(dlogit) else torch.full_like(lg, float(dlogit))
        bound = bound + p * (dl + (p * dl).sum(-1, keepdim=True))
    return p, bound


def argmax_checked(classes, logits, dlogit):
    """Compare the argmax of rows whose top-2 gap exceeds twice the logit error
    bound; returns the share of rows compared (the caller asserts it is 1.0,
    so nothing is silently skipped)."""
    lg = d(logits)
    top2 = lg.topk(2, -1).values if lg.shape[-1] > 1 else torch.cat([lg, lg - 1], -1)
    dl = d(dlogit).amax(-1) if torch.is_tensor(dlogit) else torch.full_like(top2[:, 0], float(dlogit))
    clear = (top2[:, 0] - top2[:, 1]) > 2 * dl
    got = classes.detach().cpu().reshape(-1)
    want = lg.argmax(-1)
    assert torch.equal(got[clear], want[clear]), (got, want)
    return clear.double().mean().item()


def head_ref(x, w, bias, n, ks=8):
    """Classifier head softmax(mean_hw(x) @ w^T + bias)[:, :n] -> (probs,
    bound, logits, dlogit).  The pooled row is rounded to bf16 (an MFMA
    operand) and never returned, so its rounding propagates:
        dlogit = (2^-8 |pooled| + gap_acc) |W|^T + (K + ks + 4) E (|pooled| |W|^T + |b|)
    (for HW == 1 the pooled value is the input itself: x * 1.0 is exact and
    the propagated term is zero)."""
    x, w, bias = d(x), d(w)[:n], d(bias)[:n]
    m, k = x.shape[0], x.shape[-1]
    hw = x.shape[1] * x.shape[2]
    pooled = x.reshape(m, hw, k).mean(1)
    gacc = (hw + 2) * E * x.reshape(m, hw, k).abs().mean(1)
    dp = torch.zeros_like(pooled) if hw == 1 else U_BF16 * (pooled.abs() + gacc) + gacc
    logits = pooled @ w.t() + bias
    dlogit = dp @ w.abs().t() + (k + ks + 4) * E * (pooled.abs() @ w.abs().t() + bias.abs())
    p, bound = softmax_ref(logits, dlogit)
    return p, bound, logits, dlogit


def dense_softmax_ref(x, w, bias, n):
    """softmax(x @ w[:n]^T + bias[:n]) with fp32 x (exact in fp64)."""
    pre, mag = gemm_parts(x, w[:n], None if bias is None else bias[:n])
    dlogit = (x.shape[-1] + 4) * E * mag
    p, bound = softmax_ref(pre, dlogit)
    return p, bound


def maxpool_ref(x, kh, kw, sh, sw, pt, pb, pl, pr):
    """Bit-exact: NHWC max over -inf-padded windows."""
    xp = F.pad(d(x).permute(0, 3, 1, 2), [pl, pr, pt, pb], value=float("-inf"))
    return F.max_pool2d(xp, (kh, kw), (sh, sw)).permute(0, 2, 3, 1)


def tile_shape(bm, bn):
    """One full tile plus a partial one in M, an N tail."""
    return bm + 24, bn + 8


# ---------------------------------------------------------------- shared inputs
def gemm_inputs(m, n, k, seed=0):
    """Pre-activations of standard deviation ~2: both GELU tails and the tanh
    saturation are exercised."""
    x = rnd(m, k, seed=seed + 1).to(BF)
    w = rnd(n, k, scale=1.6 / math.sqrt(k), seed=seed + 2).to(BF)
    b = rnd(n, scale=0.3, seed=seed + 3)
    r = rnd(m, n, seed=seed + 4).to(BF)
    return x, w, b, r


def conv_inputs(n, h, w, cin, cout, k, s, pads, seed=0):
    x = rnd(n, h, w, cin, seed=seed + 1).to(BF)
    wt = (rnd(k, k, cin, cout, scale=1.0 / math.sqrt(k * k * cin), seed=seed + 2)).to(BF).float()
    b = rnd(cout, scale=0.3, seed=seed + 3)
    ho = (h + pads[0] + pads[1] - k) // s + 1
    wo = (w + pads[2] + pads[3] - k) // s + 1
    r = rnd(n, ho, wo, cout, seed=seed + 4).to(BF)
    return x, wt, b, r


# (m, hw, k, np, n, seed): seeds at which every row's top-2 logit gap clears
# twice the derived logit error (argmax_checked compares 100 % of the rows)
HEAD_CASES = [(3, 4, 512, 10, 10, 40), (5, 1, 4096, 33, 33, 41), (2, 9, 512, 2000, 1500, 42)]


def head_inputs(m, hw, k, np_, seed):
    x = rnd(m, hw, 1, k, seed=seed).to(BF)
    w = rnd(np_, k, scale=0.05, seed=seed + 1).to(BF)
    b = rnd(np_, scale=0.1, seed=seed + 2)
    return x, w, b
