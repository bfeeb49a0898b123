"""Inputs, fp64 references and per-element error bounds of the fused encoder MLP (include/lthm.h
lthm_mlp_*, recommendations_amd/csrc/mlp.hip):

    pre = x W1^T + b1      h = GELU(pre)          out = bf16(h) W2T + b2 + res1 + res2
    dH  = dy W2T^T         dp = dH GELU'(pre)     dX  = bf16(dp) W1
    dW1 = bf16(dp)^T x     dW2 = dy^T bf16(h)     db1 = colsum dp

tests/test_mlp_host.py pins the references and the bounds on the CPU; tests/test_gpu_mlp_rows.py
holds every kernel of mlp.hip to them, element by element.  Plain torch on the CPU, nothing is
imported from recommendations_amd; the activations, U32, U16 and the measured term T are
tests/gemm_case.py's.

The kernels round the hidden (h, dp) to bf16 before the second product.  A worst-case 2^-8 per
hidden term would be as large as a dropped chunk, so the bound follows the rounding boundaries
(DESIGN.md section 19).  With u = 2^-23 and S = |x| |W1|^T:
  e_pre = (D + 1) u S + u |pre|                 the f32 sum of D exact products, the b1 add
  e_h   = L e_pre + T                           L: the largest |GELU'|, T: gemm_case.act_term
  e_dp  = |GELU'| e_dH + |dH| e_g' + e_dH e_g' + u |dp|,  e_dH = (D + 1) u |dy| |W2T|^T,
          e_g' = L' e_pre + T'                  L': the largest |GELU''|
If [v - e, v + e] holds no bf16 rounding boundary the device's bf16 value IS bf16(v_fp64) and
nothing reaches the second product; otherwise it is one of the two neighbours.  slack = the
distance between bf16(v - e) and bf16(v + e): 0 for an unflagged element.  Downstream:
  out, dX        slack |W|  +  (HID + 1) u |hidden_bf16| |W|      (W: W2T, W1)
  dW1, dW2       slack^T |x|, |dy|^T slack  +  (n + 1) u |a|^T |b|,  n = rows of a slice + nslice
  db1            sum e_dp  +  (n + 1) u sum |dp|                   (summed in f32 before rounding)
  + u (|terms|)  per bias / residual add;  + 2^-8 (|ref| + e) for a bf16 destination.
"""
import functools
import math
import zlib
from collections import namedtuple
from types import SimpleNamespace

import torch

import gemm_case as G
from gemm_case import U16, U32, bf

# bias: b1 and b2 present.  nres: residuals of the forward.  M rows, D model width, HID hidden.
# hot: -1, or the 32-unit hidden chunk whose W2T rows keep their scale while every other row is
# scaled by 2^-6 (a fault in that chunk then stands out of the other chunks' summation error).
Spec = namedtuple("Spec", "M D HID bias nres hot", defaults=(True, 1, -1))

LN_EPS = 1e-5
# product scale of the first layer where b1 is present: pre = b1 + (x W1^T of this deviation), so
# that e_pre, which grows with |x| |W1|^T, stays far below a bf16 step of h (module docstring)
SP = 2.0 ** -7


def _gen(*parts):
    return torch.Generator().manual_seed(zlib.crc32(repr(parts).encode()))


@functools.lru_cache(maxsize=3)
def make_case(spec):
    """The spec's tensors (bf16-rounded values held as f32 where the kernel takes bf16); shared by
    every test of the spec, do not modify.
    With b1: x ~ N(0, 1), W1 ~ N(0, SP^2 / D), |b1| ~ U(0.6, 1.6), every sixteenth negative: the hidden's
    variety comes from b1, away from 0 where a bf16 step of h falls below the radius.
    Without: x = |N(0, 1)| and W1 = |N(0, 1)| / (4 sqrt D): every product positive, S = pre."""
    M, D, HID, bias, nres, hot = spec
    g = _gen("mlp", M, D, HID, bias)
    if bias:
        x = bf(torch.randn(M, D, generator=g))
        W1 = bf(torch.randn(HID, D, generator=g) * (SP / math.sqrt(D)))
        b1 = 0.6 + torch.rand(HID, generator=g)
        # every sixteenth unit on GELU's negative branch (h < 0, GELU' < 0, dp < 0), where |GELU'| is largest
        b1[3::16] = -(0.9 + 0.3 * torch.rand(HID, generator=g)[3::16])
        b2 = 0.1 * torch.randn(D, generator=g)
    else:
        x = bf(torch.randn(M, D, generator=g).abs())
        W1 = bf(torch.randn(HID, D, generator=g).abs() / (4.0 * math.sqrt(D)))
        b1 = b2 = None
    # dy and W2T positive: dH = dy W2T^T has no cancellation, |dy| |W2T|^T = dH, so that the radius of
    # dp = dH GELU'(pre) is (D + 1) u |dp| and not 0.64 sqrt(D) times that (random signs)
    W2T = bf(torch.randn(HID, D, generator=g).abs() / math.sqrt(HID))
    if hot >= 0:
        sc = torch.full((HID, 1), 2.0 ** -6)
        sc[32 * hot:32 * hot + 32] = 1.0
        W2T = W2T * sc
    dy = bf(torch.randn(M, D, generator=g).abs())
    res = [torch.randn(M, D, generator=g) for _ in range(2)]
    return SimpleNamespace(spec=spec, x=x, W1=W1, W2T=W2T, b1=b1, b2=b2, dy=dy, res=res[:nres])


def ln_inputs(M, D, with_b):
    """f32 rows, weight and bias of the LayerNorm prologue (lthm_mlp_fwd_ln)"""
    g = _gen("ln", M, D)
    x = torch.randn(M, D, generator=g) * 0.02 + 0.5  # variance 4e-4: eps = 1e-5 is 1 % of rstd
    lw = 1.0 + 0.2 * torch.randn(D, generator=g)
    lb = 0.1 * torch.randn(D, generator=g) if with_b else None
    return x, lw, lb


def slack(v, e):
    """distance between the bf16 neighbours the interval [v - e, v + e] can round to (0: one value)"""
    return (bf(v + e) - bf(v - e)).abs()


def hidden(c, x=None, backward=False):
    """The hidden in float64 with its radii.  x: the [M, D] operand (default the case's).
    -> pre, e_pre, h, hb = bf16(h), sg (slack of h); backward: dH, dp, dpb, sd, e_dp too"""
    D = c.spec.D
    x = (c.x if x is None else x).double()
    W1 = c.W1.double()
    pre = x @ W1.t()
    e_pre = (D + 1) * U32 * (x.abs() @ W1.abs().t())
    if c.b1 is not None:
        pre = pre + c.b1.double()
        e_pre = e_pre + U32 * pre.abs()
    h = G.gelu(pre)
    e_h = G.L_GELU * e_pre + G.act_term(G.gelu, pre)
    out = SimpleNamespace(pre=pre, e_pre=e_pre, h=h, e_h=e_h, hb=bf(h), sg=slack(h, e_h))
    if backward:
        dy, W2T = c.dy.double(), c.W2T.double()
        dH = dy @ W2T.t()
        e_dH = (D + 1) * U32 * (dy.abs() @ W2T.abs().t())
        gd = G.gelu_grad(pre)
        e_gd = G.L_GELU_D * e_pre + G.act_term(G.gelu_grad, pre)
        dp = dH * gd
        e_dp = gd.abs() * e_dH + dH.abs() * e_gd + e_dH * e_gd + U32 * dp.abs()
        out.dH, out.dp, out.e_dp, out.dpb, out.sd = dH, dp, e_dp, bf(dp), slack(dp, e_dp)
    return out


def share_limit(D, bias, what):
    """The largest flagged share a case may have (what: "h" or "dp"): 1 %, or the floor where no
    input can reach 1 %.  A value v with radius e is flagged with probability 2 e / step, and a bf16
    step is 2^-8 .. 2^-7 of |v|.  A value that comes from a D-term f32 sum without a dominating bias
    has e >= (D + 1) u |v| k even with same-sign terms (S = |sum|), so its share reaches
    2 (D + 1) u 2^8 k at the worst mantissa: 0.79 % k at D = 128, 1.57 % k at D = 256.
      h  with b1: the product is 2^-7 of b1, 1 % holds.  Without: k = L (e_h = L e_pre).
      dp with b1: dH = dy W2T^T has no bias, k = 1, and a quarter more for T' and for the sixteenth of the
         units on GELU's negative branch, where |GELU'| <= 0.13 divides e_g'.  Without b1 e_g' = L' e_pre
         adds L' pre / GELU'(pre) <= 3 L' (pre in 1 .. 3.2, GELU' >= 1 there): k = 1 + 3 L'."""
    if what == "h":
        k = 0.0 if bias else G.L_GELU
    else:
        k = 1.25 if bias else 1.0 + 3.0 * G.L_GELU_D
    return max(0.01, 2 * (D + 1) * U32 * 2.0 ** 8 * k)


def share_ok(flags, limit):
    """the flagged count is within the limit, with three binomial deviations for the draw (a case
    of 32 hidden elements has a share of 0 or at least 3 %)"""
    n = flags.numel()
    return float(flags.sum()) <= limit * n + 3.0 * math.sqrt(limit * n)


def flagged_share(hid):
    """the share of hidden elements whose radius holds a bf16 rounding boundary (h; and dp)"""
    n = hid.sg.numel()
    if n == 0:
        return 0.0
    s = float((hid.sg > 0).sum()) / n
    if hasattr(hid, "sd"):
        s = max(s, float((hid.sd > 0).sum()) / n)
    return s


def second(hb, sl, W, n, out_bf16=False, adds=()):
    """ref and bound of  hb . W (+ adds)  where hb [R, K] is the bf16 hidden (float64), sl its slack,
    W [K, C] float64, n the number of f32 additions a sum passes through"""
    ref = hb @ W
    e = sl @ W.abs() + (n + 1) * U32 * (hb.abs() @ W.abs())
    mag = ref.abs()
    for t in adds:
        ref = ref + t.double()
        mag = mag + t.double().abs()
        e = e + U32 * (mag + e)
    if out_bf16:
        e = e + U16 * (ref.abs() + e)
    return ref, e


def fwd(c, x=None, hid=None):
    """lthm_mlp_fwd: -> (out float64 [M, D], its bound); x: another [M, D] operand (the LN output)"""
    hid = hidden(c, x) if hid is None else hid
    adds = ([c.b2.expand(c.spec.M, -1)] if c.b2 is not None else []) + list(c.res)
    return second(hid.hb, hid.sg, c.W2T.double(), c.spec.HID, adds=adds)


def dx(c, hid, out_bf16):
    """dX against fp64: -> (ref, bound)"""
    return second(hid.dpb, hid.sd, c.W1.double(), c.spec.HID, out_bf16=out_bf16)


def dx_from_dp(c, dP, out_bf16):
    """dX against the RETURNED dP (the operand the kernel used): only the f32 sum is left"""
    dP = dP.double()
    return second(dP, torch.zeros_like(dP), c.W1.double(), c.spec.HID, out_bf16=out_bf16)


def wgrad_n(M, nslice):
    """f32 additions a weight-gradient sum passes through: the rows of the longest slice (whole
    32-row tiles) and the fold's nslice adds"""
    tiles = -(-M // 32)
    return 32 * -(-tiles // max(nslice, 1)) + nslice


def wgrad(c, hid, nslice):
    """lthm_mlp_wgrad: -> dict name -> (ref, bound) for dW1 [HID, D], dW2 [D, HID], db1 [HID]"""
    n = wgrad_n(c.spec.M, nslice)
    x, dy = c.x.double(), c.dy.double()
    dW1, e1 = second(hid.dpb.t(), hid.sd.t(), x, n)
    r2, e2 = second(hid.hb.t(), hid.sg.t(), dy, n)
    db1 = hid.dp.sum(0)
    eb = hid.e_dp.sum(0) + (n + 1) * U32 * hid.dp.abs().sum(0)
    return {"dW1": (dW1, e1), "dW2": (r2.t(), e2.t()), "db1": (db1, eb)}


def hidden_ratio(got, refb, sl):
    """G / dP: max |got - bf16(ref)| / slack; inf where an unflagged element differs at all"""
    d = (got.double() - refb).abs()
    if d.numel() == 0:
        return 0.0
    if not bool(torch.isfinite(d).all()) or bool(((sl == 0) & (d > 0)).any()):
        return float("inf")
    return float((d / sl.clamp_min(1e-300)).max())


HIDDEN_OK = 1.0 + 2.0 ** -20  # hidden_ratio below this: every element within its slack


def ratio(got, ref, bnd):
    if ref.numel() == 0:
        return 0.0
    return G.ratio(got, ref, bnd)


# ----------------------------------------------------------------------------- LayerNorm prologue
def ln(x, lw, lb):
    """mean, rstd and the normalised rows y (before the bf16 store) in float64 with bounds, for
    mlp_load_ln's two-pass arithmetic: s = f32 sum of D values (D + 1 additions with the lane
    exchange), mu = s / D; q = f32 sum of (v - mu)^2; rs = 1 / sqrt(q / D + eps);
    y = (v - mu) rs w + b.
      e_mu = (D + 2) u mean|x|
      e_d  = e_mu + u |v - mu|                          per deviation
      e_q  = D e_mu^2 + sum (2 a r + r^2 + u a^2) + (D + 1) u (q + D e_mu^2),  a = |d| + e_mu,
             r = u a: the mean's error t shifts every deviation alike and sum d = 0, so
             sum (d - t)^2 = q + D t^2 exactly; only each subtraction's own rounding r is linear
      e_rs = rs (e_q / D / (2 (var + eps)) + 8 u)       division, square root, reciprocal
      e_y  = |w| (|rs| e_d + |d| e_rs + e_d e_rs) + 4 u (|y| + |b|)
    h = bf16(y): within e_y + 2^-8 (|y| + e_y) of y."""
    D = x.shape[1]
    xd, w = x.double(), lw.double()
    mu = xd.mean(1)
    e_mu = (D + 2) * U32 * xd.abs().mean(1)
    d = xd - mu[:, None]
    e_d = e_mu[:, None] + U32 * d.abs()
    q = (d * d).sum(1)
    a = d.abs() + e_mu[:, None]
    r = U32 * a
    shift = D * e_mu * e_mu
    e_q = shift + (2 * a * r + r * r + U32 * a * a).sum(1) + (D + 1) * U32 * (q + shift)
    var = q / D
    rs = 1.0 / torch.sqrt(var + LN_EPS)
    e_rs = rs * (e_q / D / (2 * (var + LN_EPS)) + 8 * U32)
    y = d * rs[:, None] * w
    b = lb.double() if lb is not None else torch.zeros(D, dtype=torch.float64)
    y = y + b
    e_y = w.abs() * (rs[:, None] * e_d + d.abs() * e_rs[:, None] + e_d * e_rs[:, None]) + 4 * U32 * (y.abs() + b.abs())
    e_h = e_y + U16 * (y.abs() + e_y)
    return SimpleNamespace(mean=mu, e_mean=e_mu, rstd=rs, e_rstd=e_rs, y=y, e_h=e_h)


# ----------------------------------------------------------------------------- the CPU evaluation
def evaluate_f32(c, nslice=1):
    """The kernels' arithmetic in float32 on the CPU: bf16 operands, f32 sums over the hidden in
    32-unit chunk order, h / dp rounded to bf16; the weight gradients per token slice, folded."""
    M, D, HID = c.spec[:3]
    x, dy, W1, W2T = c.x, c.dy, c.W1, c.W2T
    pre = x @ W1.t()
    if c.b1 is not None:
        pre = pre + c.b1
    h, gd = G.gelu(pre), G.gelu_grad(pre)
    hb = bf(h)
    dp = (dy @ W2T.t()) * gd
    dpb = bf(dp)
    out = torch.zeros(M, D)
    dX = torch.zeros(M, D)
    for j in range(0, HID, 32):
        out = out + hb[:, j:j + 32] @ W2T[j:j + 32]
        dX = dX + dpb[:, j:j + 32] @ W1[j:j + 32]
    t = torch.zeros(M, D)
    if c.b2 is not None:
        t = t + c.b2
    for r in c.res:
        t = t + r
    out = out + t
    tiles = -(-M // 32)
    dW1, dW2T, db1 = torch.zeros(HID, D), torch.zeros(HID, D), torch.zeros(HID)
    for s in range(nslice):
        lo, hi = 32 * (tiles * s // nslice), min(M, 32 * (tiles * (s + 1) // nslice))
        dW1 = dW1 + dpb[lo:hi].t() @ x[lo:hi]
        dW2T = dW2T + hb[lo:hi].t() @ dy[lo:hi]
        db1 = db1 + dp[lo:hi].sum(0)
    return SimpleNamespace(out=out, G=hb, dP=dpb, dX=dX, dW1=dW1, dW2=dW2T.t().contiguous(), db1=db1)


# ----------------------------------------------------------------------------- the GPU cases
def fwd_specs(cus):
    """lthm_mlp_fwd / lthm_mlp_fwd_ln: the row edges of the 256-row tile x NC = 1, 2, 3, 4, 32, both
    widths, bias none / both and 0 / 1 / 2 residuals at both; two rows-by-CU cases per HID where
    every workgroup walks a full tile, then a ragged one with idle waves; the largest HID."""
    s = [Spec(1, 128, 32, True, 0), Spec(31, 256, 64, True, 1), Spec(32, 128, 96, False, 2),
         Spec(33, 256, 128, True, 2), Spec(255, 128, 1024, True, 1), Spec(256, 256, 32, True, 1),
         Spec(257, 128, 64, False, 1), Spec(1000, 256, 96, True, 2), Spec(257, 256, 1024, True, 1),
         Spec(1000, 128, 128, False, 0), Spec(33, 256, 96, False, 0), Spec(256, 128, 128, True, 1),
         Spec(257, 256, 64, False, 1),
         Spec(255, 256, 64, True, 2), Spec(32, 256, 1024, True, 1, 31), Spec(1, 256, 96, True, 1),
         Spec(31, 128, 32, True, 2), Spec(257, 128, 1024, True, 1, 5)]
    s += [Spec(cus * 296, D, HID, True, 1) for D in (128, 256) for HID in (64, 96)]
    s += [Spec(33, 128, 8192, True, 1, 255), Spec(33, 256, 7424, True, 1, 231), Spec(0, 256, 64, True, 1)]
    return s


def bwd_specs(cus, fused):
    """lthm_mlp_bwd_hidden + dgrad (256-row tiles) / lthm_mlp_bwd (128-row tiles)"""
    ms = (1, 31, 32, 33, 127, 128, 129, 255, 256, 257, 1000)
    hs = (32, 96, 1024)
    s = [Spec(M, (128, 256)[i % 2], hs[i % 3], i % 4 != 2, 0) for i, M in enumerate(ms)]  # b1 = None: 32, 129, 1000
    s += [Spec(33, 256, 4128, True, 0), Spec(33, 128, 8192, True, 0)]
    s += [Spec(cus * ((128 if fused else 256) + 40), 256, 64, True, 0)]
    return s


def bwd_dx_specs(cus):
    s = [Spec(M, (128, 256)[(i + k) % 2], HID, (i + k) % 5 != 4, 0) for i, HID in enumerate((32, 64, 96, 128, 160))
         for k, M in enumerate((5, 128, 129))]  # b1 = None at (96, 129), (128, 128), (160, 5)
    s += [Spec(cus * 168, D, HID, True, 0) for D in (128, 256) for HID in (32, 96, 160)]
    return s


def wgrad_ms(ns):
    """lthm_mlp_wgrad: M with 1, 2, 3, 4 and an uneven 4 / 5 token tiles per slice for a device whose
    plan gives `ns` slices, each tile count once whole (M % 32 == 0, FULL) and once ragged
    (M % 32 in {1, 19}), then M = 5"""
    ms = []
    for k, rag in ((1, 0), (1, 19), (2, 0), (2, 1), (3, 0), (3, 19), (4, 0), (4, 1)):
        ms.append(32 * ns * k - (32 - rag if rag else 0))
    half = ns * 4 + ns // 2 if ns > 1 else 5
    return ms + [32 * half, 32 * half - 13, 5]


WGRAD_FORMS = [(128, 128, True, True), (256, 128, False, True), (256, 4096, True, False), (128, 4096, True, True)]
