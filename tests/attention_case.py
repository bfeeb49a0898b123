"""Inputs, fp64 references and the per-row error bounds of the attention kernels
(tests/test_attention_host.py pins the references on the CPU, tests/test_gpu_attention.py holds
the kernels of recommendations_amd/csrc/attention.hip to them).

Everything here is plain torch on the CPU.  Nothing is imported from recommendations_amd: the
formulas restate commons/transformers/layers.py:49-61 (SDPA with the relative-position bias
table[q - k + T, h], an additive mask and the causal rule) and its hand-derived backward.

Tensors are [B, H, T, E] (q, k, v, dout, out and the gradients), lse is [B, H, T], the table is
[2T + 5, H] (the kernels read rows 0 .. 2T) and its gradient [2T + 1, H].  With mqa the case's
k and v are [B, 1, T, E], one head shared by all query heads, and dk / dv are the sums over the
heads.

The bounds of the GPU tests come from these references alone (bounds()):
  out, dq, dk, dv   4 x max over rows of row_err(bf16_model, reference)
  dtable            the same per table row, over the H axis
  lse               8 x max |lse evaluated in float32 on the CPU - reference|
"""
import functools
import math
from collections import namedtuple
from types import SimpleNamespace

import numpy as np
import torch

MASK_KINDS = (None, "T,T", "B,1", "1,H", "B,H")

Spec = namedtuple("Spec", "B T H E causal table mask_kind scale mqa", defaults=(True, None, 1.0, False))


def _seed(s):
    return (((s.B * 4099 + s.T) * 17 + s.H) * 257 + s.E) * 64 + 32 * int(s.causal) + 16 * int(s.table) \
        + 2 * MASK_KINDS.index(s.mask_kind) + int(s.mqa)


def bf(x):
    """round to bf16 (nearest even), keep the dtype"""
    return x.to(torch.bfloat16).to(x.dtype)


def make_case(B, T, H, E, causal, table, mask_kind, seed, scale=1.0, mqa=False):
    """bf16-rounded q, k, v, dout (held as f32), the optional f32 table [2T + 5, H] and the
    optional f32 mask.  scale multiplies q before the rounding (the softmax-range cases).

    Masks: random finite scores (sigma = 1) plus -inf on a random set of about 10 % of the keys,
    one set per batch entry (one in all for the kinds without a batch axis), never empty.  Key 0 is never
    masked: under the causal rule it is the only key row 0 sees, so every (b, h, q) row keeps a
    finite key -- asserted below; fully masked rows are out of scope (the reference gives NaN)."""
    assert mask_kind in MASK_KINDS
    g = torch.Generator().manual_seed(seed)
    Hkv = 1 if mqa else H
    q = bf(scale * torch.randn(B, H, T, E, generator=g))
    k = bf(torch.randn(B, Hkv, T, E, generator=g))
    v = bf(torch.randn(B, Hkv, T, E, generator=g))
    dout = bf(torch.randn(B, H, T, E, generator=g))
    tab = 0.5 * torch.randn(2 * T + 5, H, generator=g) if table else None
    mask = None
    if mask_kind is not None:
        mb, mh = {"T,T": (1, 1), "B,1": (B, 1), "1,H": (1, H), "B,H": (B, H)}[mask_kind]
        mask = torch.randn(mb, mh, T, T, generator=g)
        dead = torch.rand(mb, 1, 1, T, generator=g) < 0.1
        dead[..., 0] = False
        if T > 2:  # every set masks at least one key
            dead[..., T // 2] |= ~dead.any(-1)
        mask = mask.masked_fill(dead.expand(mb, mh, T, T), -float("inf"))
        if mask_kind == "T,T":
            mask = mask[0, 0]
    c = SimpleNamespace(B=B, T=T, H=H, E=E, causal=bool(causal), q=q, k=k, v=v, dout=dout, table=tab, mask=mask,
                        mask_kind=mask_kind, mqa=bool(mqa), scale=scale)
    S = scores(c, torch.float32)
    assert bool(torch.isfinite(S).any(-1).all()), "a fully masked row"
    return c


def case_of(spec):
    return make_case(spec.B, spec.T, spec.H, spec.E, spec.causal, spec.table, spec.mask_kind, _seed(spec),
                     scale=spec.scale, mqa=spec.mqa)


def rel_pos(T):
    """table row of (q, k): q - k + T"""
    return torch.arange(T)[:, None] - torch.arange(T)[None, :] + T


def scores(c, dtype):
    """S[b, h, q, k] = q . k / sqrt(E) + table[q - k + T, h] + mask, -inf above the diagonal"""
    T = c.T
    S = c.q.to(dtype) @ c.k.to(dtype).transpose(-1, -2) / math.sqrt(float(c.E))
    if c.table is not None:
        S = S + c.table.to(dtype)[rel_pos(T)].permute(2, 0, 1)[None]
    if c.mask is not None:
        S = S + c.mask.to(dtype)
    if c.causal:
        S = S.masked_fill(torch.ones(T, T, dtype=torch.bool).triu(1), -float("inf"))
    return S


def lse_f32(c):
    """the lse formula evaluated in float32 on the CPU: its distance from the fp64 lse is the
    unit of the lse bound"""
    return torch.logsumexp(scores(c, torch.float32), -1)


def _eval(c, r, ri):
    """Forward and backward in float64 by explicit formulas; r rounds what is stored, ri what
    enters a second product (P, dS), where bf16_model says."""
    f64 = torch.float64
    T, E = c.T, c.E
    rs = 1.0 / math.sqrt(float(E))
    q, k, v, do = c.q.to(f64), c.k.to(f64), c.v.to(f64), c.dout.to(f64)
    S = scores(c, f64)
    lse = torch.logsumexp(S, -1)
    P = torch.exp(S - lse[..., None])
    del S
    Pr = ri(P)
    out = r(Pr @ v)
    delta = (do * out).sum(-1)
    dS = P * (do @ v.transpose(-1, -2) - delta[..., None])
    del P
    dS = ri(dS)
    dq = r(dS @ k * rs)
    dk = r(dS.transpose(-1, -2) @ q * rs)
    dv = r(Pr.transpose(-1, -2) @ do)
    del Pr
    if c.mqa:  # the caller's expand-and-sum: per-head gradients, summed over the heads
        dk, dv = dk.sum(1, keepdim=True), dv.sum(1, keepdim=True)
    dtable = None
    if c.table is not None:
        dtable = torch.zeros(c.H, 2 * T + 1, dtype=f64)
        dtable.index_add_(1, rel_pos(T).reshape(-1), dS.sum(0).reshape(c.H, T * T))
        dtable = dtable.t().contiguous()
    return SimpleNamespace(out=out, lse=lse, dq=dq, dk=dk, dv=dv, dtable=dtable)


def reference(c):
    """float64, no rounding anywhere:
      S, lse = logsumexp_k S, P = exp(S - lse), O = P V,
      delta = rowsum(dO o O), dS = P o (dO V^T - delta),
      dQ = dS K / sqrt(E), dK = dS^T Q / sqrt(E), dV = P^T dO,
      dtable[i, h] = sum of dS over the batch and q - k + T = i
    (mqa: K / V shared, dK / dV summed over the heads)."""
    return _eval(c, lambda x: x, lambda x: x)


def bf16_model(c):
    """The same formulas with the bf16 roundings of the MFMA kernels (attention.hip):
      * P before P V (attn_fwd_mfma_k, attn_fwd32_k and attn_fwd_win_k feed P to the second MFMA
        as bf16 hi + lo halves: about 16 bits, the model keeps 8) and before P^T dO;
      * dS before dS K and dS^T Q (attn_bwd32_k, attn_bwd32l_k: one bf16 straight from the
        accumulator; attn_bwd_mfma_k and the windowed kernels: hi + lo);
      * O on store, and so O as the backward re-reads it for delta = rowsum(dO o O);
      * dQ, dK, dV on store (mqa: each head's dK / dV, before the f32 sum over the heads).
    Scores, lse, dP = dO V^T and delta stay unrounded (f32 in the kernels).  The bias gradient is
    summed from the f32 dS in every kernel; the model sums the rounded dS.  It is an upper model of
    the rounding, not an emulation, and the factor 4 of the bounds covers what it leaves out (f32
    accumulation order, exp2 / log2 approximations, atomics order).

    The whole-head VALU kernels (attn_fwd_k / attn_bwd_k: E = 16, or any mask) keep P and dS in
    f32, and for the cases they serve the model leaves P and dS unrounded too (valu_served).
    Rounding there anyway is not an upper model: a dq row with few keys and a norm under the floor
    of row_err is carried by the error of delta = rowsum(dO o bf16(O)), a single draw that moves
    with every bf16 value of O.  At (2, 65, 2, 16, causal, table) row (1, 0, 1) the stores alone
    give 6.05e-2, which is what attn_bwd_k returns, and the model with P rounded 5.3e-3, because
    its O lands on other bf16 values."""
    return _eval(c, bf, (lambda x: x) if valu_served(c) else bf)


def valu_served(c):
    """attn_dispatch: a mask, or E = 16, goes to the whole-head VALU kernels (T <= 256)"""
    return c.mask is not None or c.E == 16


def row_err(got, want):
    """Per-row error over the last axis: |got - want| / max(|want|, 1e-2 max_row |want|), as a
    tensor over the leading axes (argmax names the worst (b, h, t)).  The floor keeps rows whose
    reference is exactly zero (the causal row 0 of dq) from dividing by zero and still bounds them
    to 1e-2 x bound of the largest row."""
    got, want = got.double(), want.double()
    wn = want.norm(dim=-1)
    floor = 1e-2 * float(wn.max())
    if floor == 0.0:
        raise ValueError("the reference is all zero: no relative error (see zero_bound)")
    return (got - want).norm(dim=-1) / wn.clamp_min(floor)


def worst(err):
    """(max, index) of a row_err tensor"""
    i = int(torch.argmax(err))
    return float(err.reshape(-1)[i]), tuple(int(x) for x in np.unravel_index(i, tuple(err.shape)))


def zero_tensors(spec):
    """Reference tensors that are exactly zero: with one key the softmax is 1 whatever the
    scores, so dS = 0 and with it dq, dk and dtable."""
    return ("dq", "dk", "dtable") if spec.T == 1 else ()


def zero_bound(c):
    """T = 1: max |element| a correct kernel may leave in dq, dk and dtable.  p = 1 exactly and
    O = V exactly (bf16), so dS = dO . V - dO . O is the difference of two f32 dot products of the
    same E terms in different orders: |dS| <= 2 E 2^-24 sum|dO V|; times |k| or |q| / sqrt(E)
    and the bf16 store (1 + 2^-8) for dq and dk, summed over the batch for dtable."""
    ds = 2.0 * c.E * 2.0 ** -24 * float((c.dout.double() * c.v.double()).abs().sum(-1).max())
    g = ds * (1.0 + 2.0 ** -8) / math.sqrt(float(c.E))
    return {"dq": g * float(c.k.abs().max()), "dk": g * float(c.q.abs().max()), "dtable": c.B * ds}


TENSORS = ("out", "dq", "dk", "dv")
# T = 1: out = V and dv = dO are bf16 values, the model's roundings change nothing and 4 x its
# error is 0.  A kernel that reaches them through p / l with approximate exp and reciprocal may
# be one bf16 ulp off in an element, so these two are held to 2^-8 per row instead.
EXACT_AT_T1 = ("out", "dv")


@functools.lru_cache(maxsize=None)
def bounds(spec):
    """(case, reference, model maxima, bounds) of one spec, computed once per session and never
    changed.  model maxima: max over rows of row_err(bf16_model, reference) for out / dq / dk /
    dv / dtable, max |model - reference| for the same (the softmax-range gradients), and
    max |lse_f32 - reference lse| for lse."""
    c = case_of(spec)
    ref, mod = reference(c), bf16_model(c)
    zero = zero_tensors(spec)
    names = TENSORS + (("dtable",) if c.table is not None else ())
    mmax, amax = {}, {}
    for n in names:
        w, m = getattr(ref, n), getattr(mod, n)
        amax[n] = float((m - w).abs().max())
        if n in zero:
            assert float(w.abs().max()) == 0.0, n
            continue
        mmax[n] = float(row_err(m, w).max())
    mmax["lse"] = float((lse_f32(c).double() - ref.lse).abs().max())
    # half an f32 ulp of the largest lse: no f32 result is held closer than that.  It takes over
    # where few short rows leave the CPU's f32 evaluation exact or nearly so (T = 1, T = 21)
    lse_floor = 2.0 ** -24 * float(ref.lse.abs().max())
    mmax["lse"] = max(mmax["lse"], lse_floor)
    bnd = {n: (8.0 if n == "lse" else 4.0) * e for n, e in mmax.items()}
    for n in EXACT_AT_T1 if spec.T == 1 else ():
        assert mmax[n] == 0.0, n
        bnd[n] = 2.0 ** -8
    return SimpleNamespace(spec=spec, case=c, ref=ref, model_max=mmax, model_abs=amax, bound=bnd, zero=zero,
                           lse_floor=lse_floor)


# ------------------------------------------------------------------ the case lists
def _both(cases):
    return [Spec(*c, table=t) for c in cases for t in (True, False)]


# a. one case per dispatcher branch (B, T, H, E, causal), each with and without the table
MATRIX = _both([
    # whole-head VALU kernels, E = 16, NK = 1 .. 4
    (2, 1, 2, 16, True), (2, 65, 2, 16, True), (1, 193, 1, 16, False), (2, 256, 1, 16, True),
    # attn_fwd_mfma_k / attn_bwd_mfma_k, E = 32 and 128
    (2, 31, 2, 32, True), (2, 33, 2, 32, False), (1, 256, 2, 32, False), (2, 95, 1, 128, False),
    (1, 256, 1, 128, True), (1, 256, 1, 128, False),
    # attn_fwd32_k / attn_bwd32_k, E = 64 (tail mode at causal T = 32 n + 1)
    (2, 32, 2, 64, True), (2, 33, 2, 64, True), (2, 33, 2, 64, False), (2, 65, 1, 64, True),
    (1, 255, 2, 64, True), (1, 256, 2, 64, False),
    # windowed, E = 64: fwd32 from 4 to 8 waves, attn_bwd32l_k, then the *_win_k kernels
    (1, 257, 2, 64, True), (1, 330, 1, 64, False), (1, 552, 1, 64, True), (1, 553, 1, 64, False),
    (1, 641, 1, 64, True),
    # windowed, E = 32 and 128
    (1, 257, 2, 32, False), (2, 289, 1, 128, False), (1, 1025, 1, 32, True),
]) + [
    # the length ceiling
    Spec(1, 2049, 1, 64, False, table=True), Spec(1, 2049, 1, 64, False, table=False),
    Spec(1, 4096, 1, 32, True, table=True),
]

# b. general additive masks (whole-head VALU kernels): each kind, then NK = 2, 3, 4 and every E
MASKS = [Spec(3, 21, 2, 32, True, table=True, mask_kind=kind) for kind in MASK_KINDS[1:]] + [
    Spec(2, 70, 2, 16, False, table=True, mask_kind="B,H"),
    Spec(2, 130, 3, 32, True, table=True, mask_kind="1,H"),
    Spec(1, 200, 2, 64, False, table=True, mask_kind="B,1"),
    Spec(1, 256, 1, 64, True, table=True, mask_kind="T,T"),
    Spec(2, 149, 1, 128, True, table=True, mask_kind="B,H"),
]
# the masked (T, E) limit: E = 128 holds up to T = 149
MASK_REFUSED = [(1, 150, 1, 128), (1, 256, 1, 128)]

# c. multi-query forward (K / V head stride 0, token stride 2E); the first two with the backward
MQA = [
    Spec(2, 40, 4, 32, True, table=True, mqa=True),                     # attn_fwd_mfma_k
    Spec(2, 129, 4, 64, True, table=True, mqa=True),                    # attn_fwd32_k
    Spec(1, 96, 2, 128, False, table=False, mqa=True),                  # attn_fwd_mfma_k
    Spec(2, 100, 4, 16, True, table=True, mask_kind="B,H", mqa=True),   # VALU, NK = 2
    Spec(1, 300, 2, 64, True, table=False, mqa=True),                   # windowed (fwd32, 8 waves)
    Spec(1, 300, 2, 32, False, table=True, mqa=True),                   # attn_fwd_win_k
]
MQA_BACKWARD = MQA[:2]

# d. softmax range: q scaled so that max |score| is in [100, 200] (f32 exp overflows at 88)
RANGE_SCALE = 32.0
RANGE = [
    Spec(1, 130, 1, 64, True, table=True, scale=RANGE_SCALE),
    Spec(1, 300, 1, 32, False, table=True, scale=RANGE_SCALE),
    Spec(1, 100, 1, 16, False, table=True, mask_kind="B,H", scale=RANGE_SCALE),
    Spec(1, 600, 1, 64, True, table=True, scale=RANGE_SCALE),
]

# e. guard rows round every output
GUARD = [
    Spec(3, 33, 2, 64, True, table=True), Spec(2, 47, 3, 32, True, table=True),
    Spec(3, 21, 1, 16, False, table=True, mask_kind="B,1"), Spec(2, 257, 1, 64, True, table=True),
    Spec(3, 289, 1, 128, False, table=True),
]

ALL = MATRIX + MASKS + MQA + RANGE + GUARD


def spec_id(s):
    return (f"{s.B}x{s.T}x{s.H}x{s.E}-{'causal' if s.causal else 'full'}-{'table' if s.table else 'notable'}"
            + (f"-mask{s.mask_kind.replace(',', '')}" if s.mask_kind else "") + ("-mqa" if s.mqa else "")
            + (f"-x{s.scale:g}" if s.scale != 1.0 else ""))
