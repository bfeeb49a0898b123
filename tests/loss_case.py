"""Inputs, fp64 reference, rounding model and per-row bounds of the contrastive-loss kernels
(tests/test_loss_host.py pins the reference on the CPU, tests/test_gpu_loss_rows.py holds every
dispatch path of recommendations_amd/csrc/loss.hip to it).

Everything here is plain torch / numpy on the CPU.  Nothing is imported from recommendations_amd:
the formulas restate oracle/lthm_ref.py::contrastive_loss (the reference's wrapper.py:78-245) and
its hand-derived backward.

Shapes: y [B, T + 1, NH, De] (next_token_emb), t [B, T, De] (current_token_emb), mask [B, T]
(True = pad), offsets [n_mb, NH], logq None or f32 [B, T] (the additive correction of every input
token).  Per mini-batch mb (sequences b0 .. b0 + Bm - 1) and head h with offset o, L = T - o:

  rows r = b L + t (t < L):  out_r = y^[b0 + b, t, h]          (y^ = y / |y|)
  cols c = b' L + t':        in_c  = t^[b0 + b', t' + o],  pad_c = mask[b0 + b', t' + o]
  S[r, c] = out_r . in_c / tau, excluded (-inf) where r and c share a sequence and r != c, where
  c is a pad, and where r is a pad (the pad flag of row r is pad_r: rows and columns share it);
  cnt_r = #finite S[r, :],  pos_r = S[r, r],  rank_r = #{c != r: S[r, c] > S[r, r]} (plain logits),
  lse_r = logsumexp_c (S[r, c] + [c != r] logq_c)   (the correction enters the CE only),
  used_r = not pad_r and cnt_r - 1 > 0,  CE_r = lse_r - pos_r,  U = #used,
  loss = sum_mb sum_h mean_used CE / n_mb.

The per-row outputs of the kernels are [NH, n_mb, n_max] (n_max = mbs T rounded up to 64), indexed
by r in every path.  The statistics row of a (head, mini-batch) is stats[h, mb, :] (cl_stats_k):

  ST_CE      0  mean CE over the used rows          ST_RANK    4  mean rank
  ST_USED    1  U (the effective batch)             ST_MEDIAN  5  median rank (torch.quantile 0.5)
  ST_NEG     2  mean negatives cnt - 1              ST_OFFSET  6  the offset o
  ST_MINNEG  3  min negatives (0 when U = 0)        ST_TOKENS  7  used rows with a finite CE (= U here)
  ST_HITS    8 + q  #{rank < min(ks[q], min negatives)} / U

Backward, with w_r = used_r g / (U n_mb) and P = softmax of the corrected logits:
  dS = w (P - I),  dOut_r = sum_c dS[r, c] in_c / tau,  dIn_c = sum_h sum_r dS[r, c] out_r / tau,
both through the F.normalize backward dx = (G - x^ (x^ . G)) / |x|.  Pad rows of dt and dy[:, T]
are zero, as is every dy row (b, t, h) with t >= L.

What cl_rowstats_k reads of a row that is not used (loss.hip): for r < n it reads cnt[r] before
the pad test and takes the row iff `!pad && cnt - 1 > 0`; lse, pos and rank are read of used rows
only.  So the kernels owe, besides the used rows' four values, cnt == 1 on every non-pad row
without a negative; nothing is relied on for pad rows and for n <= r < n_max (the compact path
never writes them), and the GPU tests compare nothing there.

Bounds (bounds(), from the reference and the model alone):
  dy, dt       per row, 4 x max over rows of row_err(bf16_model, reference); row_err floors a row
               at FLOOR of the largest row after dividing every row by its weight scale
  lse          8 x max |lse evaluated in float32 on the CPU - reference|, at least half an f32 ulp
               of the largest |lse|
  pos          one f32 ulp of 1 / tau
  cnt, rank, used, and the count-valued statistics (ST_USED, ST_MINNEG, ST_MEDIAN, ST_OFFSET,
  ST_TOKENS)   exact (the median of integers is an integer or a half)
  ST_NEG, ST_RANK, ST_HITS   1e-6 relative (f64 sums of exact values, stored in f32)
  ST_CE        lse bound + pos bound + 1e-6 |CE| (a mean of f32 lse - pos values)
  loss         NH (lse bound + pos bound) + 1e-6 |loss|: it is the sum over the heads of the
               means of lse - pos, averaged over the mini-batches; where the CE is of the size of
               the lse this is the lse bound taken relatively, and it stays meaningful on the rows
               whose CE cancels to e^-80.
"""
import functools
import os
import sys
from collections import namedtuple
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from contrastive_inputs import exact_unit_vectors  # noqa: E402

DE = 128
ST_CE, ST_USED, ST_NEG, ST_MINNEG, ST_RANK, ST_MEDIAN, ST_OFFSET, ST_TOKENS, ST_HITS = range(9)
EXACT_STATS = (ST_USED, ST_MINNEG, ST_MEDIAN, ST_OFFSET, ST_TOKENS)
MEAN_STATS = (ST_NEG, ST_RANK)  # and every ST_HITS + q

# floor of row_err, as a fraction of the largest row after every row is divided by its scale
# (row_err: the row weight of its (mini-batch, head) over the norm of its input row).  On that scale
# a typical row is 1 / tau x 0.7 .. 1 of the largest in every (mini-batch, head), so the floor only
# catches rows whose gradient cancels: a confident softmax (P_rr near 1; geo row (0, 209, 0) at 2 %
# of the largest, the U = 2 pair of m-left at 1 %) and the softmax-range rows at P_rr = 1 - e^-80.
# These keep an absolute model error of about 2^-9 w, and with the attention suite's 1e-2 the model
# alone reaches 1.2e-1 (m-left), 8.1e-2 (geo) and 2.4e-1 (adv-tau0.01); at 5e-2 still 4.8e-2, so 4 x
# that breaks the 0.1 cap.  At 1e-1 the worst model row of any case is 2.41e-2 (adv-tau0.01), and
# test_loss_host.py asserts 4 x model <= 0.1 and the error allowed to the median row of every
# (mini-batch, head) for every case.
FLOOR = 1e-1

TAU_LAST_FIXED = 0.025  # 2 / tau == 80 in f32 and f64: the last temperature of the fixed shift
TAU_FIRST_RUNNING = float(np.nextafter(np.float32(0.025), np.float32(0.0)))  # the f32 below it


def takes_fixed_shift(tau, logq=False):
    """The dispatcher's own expressions: lthm_contrastive_fwd / _bwd evaluate `2.f / tau <= 80.f` in
    f32 on the f32 tau, ContrastiveLossFn.forward `2.0 / tau <= 80.0` in f64 on the Python float.
    Returns (kernel side, wrapper side); a case is valid only where both agree."""
    k = bool(np.float32(2.0) / np.float32(tau) <= np.float32(80.0)) and not logq
    w = bool(2.0 / tau <= 80.0) and not logq
    return k, w


def bf(x):
    """round to bf16 (nearest even), keep the dtype"""
    return x.to(torch.bfloat16).to(x.dtype)


# ------------------------------------------------------------------ cases
# valid: None (no pads) or a tuple of per-sequence valid-token counts; pads: "left" (the valid
# tokens are the last ones) or "mixed" (the valid positions are drawn at random: interior pads).
# adv: the softmax-range construction of make_case.  g: the upstream gradient.
Spec = namedtuple("Spec", "name B T NH mbs tau offs valid pads adv logq ks ydt tdt g seed",
                  defaults=(None, "left", False, False, (1, 5, 10, 5000), "bf16", "f32", 1.0, 0))


def _exact(rng, rows, lo=-3, hi=4):
    """[rows, DE] f64: exact unit vectors (integers, sum of squares 65,536) x random powers of two"""
    v = exact_unit_vectors(rng, rows, DE).astype(np.float64)
    return v, np.exp2(rng.integers(lo, hi, size=(rows, 1))).astype(np.float64)


def make_case(s):
    """The inputs of a Spec.  Every vector is k 2^e with k an integer vector of sum of squares
    65,536 and |k_i| < 256: norms, normalised bf16 operands and logits are exact in f32 on both
    sides, so cnt and rank are exact integers, ties included.

    adv (mbs = 3, at least two mini-batches): with v one exact vector,
      mini-batch 0: t rows of sequence 0 = v, of sequence 1 = -v, sequence 2 all pad; the y rows at
        even t (every head) = v.  Even rows of sequence 0: positive at cos +1 and every negative
        at -1 (a); even rows of sequence 1: positive at -1, every negative at +1, and pad columns
        whose zero logit lies above the positive (b);
      mini-batch 1: t rows of sequence 0 = v, of sequences 1 and 2 = -v (sequence 2 with 5 left
        pads); y rows at even t = v, at t = 1 mod 4 = -v.  Rows of sequences 1 and 2 then have
        negatives that tie with the positive exactly, below other negatives (even t) and at the
        top (t = 1 mod 4) (c);
      mini-batch 2: the t rows of sequence 7 are those of sequence 8 (the same items in two
        sequences): every row of both has one negative whose dot equals the positive's at a generic
        value a, where acc * (1 / tau) and acc / tau round differently once 1 / tau is inexact (d);
      every other y row stays random."""
    rng = np.random.default_rng(1000 + s.seed)
    B, T, NH = s.B, s.T, s.NH
    yv, ys = _exact(rng, B * (T + 1) * NH)
    tv, ts = _exact(rng, B * T)
    yv, tv = yv.reshape(B, T + 1, NH, DE), tv.reshape(B, T, DE)
    mask = np.zeros((B, T), dtype=bool)
    if s.valid is not None:
        assert len(s.valid) == B
        for b, v in enumerate(s.valid):
            if s.pads == "left":
                mask[b, :T - v] = True
            else:
                mask[b] = True
                mask[b, rng.permutation(T)[:v]] = False
    if s.adv:
        assert s.mbs == 3 and B >= 6
        v = tv[0, 0].copy()
        tv[0], tv[1], mask[2] = v, -v, True
        tv[3], tv[4], tv[5] = v, -v, -v
        mask[5, :5] = True
        yv[0:6, 0:T:2] = v
        yv[3:6, 1:T:4] = -v
        tv[7] = tv[8]
    y = torch.from_numpy((yv.reshape(-1, DE) * ys).reshape(B, T + 1, NH, DE))
    t = torch.from_numpy((tv.reshape(-1, DE) * ts).reshape(B, T, DE))
    y = y.to(torch.bfloat16 if s.ydt == "bf16" else torch.float32)
    t = t.to(torch.bfloat16 if s.tdt == "bf16" else torch.float32)
    logq = None
    if s.logq:  # -beta logQ with beta = 0.7 and logQ up to 9.2, both signs: spread over +-6.44
        logq = torch.from_numpy((0.7 * (rng.random((B, T)) * 18.4 - 9.2)).astype(np.float32))
    n_mb = (B + s.mbs - 1) // s.mbs
    offs = np.asarray(s.offs, dtype=np.int32).reshape(n_mb, NH)
    return SimpleNamespace(y=y, t=t, mask=torch.from_numpy(mask), offs=offs, mbs=s.mbs, tau=float(s.tau),
                           ks=tuple(s.ks), logq=logq, g=float(s.g))


def geometry(c):
    """(B, T, NH, n_mb, n_max) of a case"""
    B, Tp, NH, _ = c.y.shape
    T = Tp - 1
    return B, T, NH, (B + c.mbs - 1) // c.mbs, ((c.mbs * T + 63) // 64) * 64


def valid_counts(c):
    """m[mb][h]: the valid rows of each (mini-batch, head), what the compact path tiles on"""
    B, T, NH, n_mb, _ = geometry(c)
    return [[int((~c.mask[mb * c.mbs:(mb + 1) * c.mbs, int(c.offs[mb, h]):]).sum()) if c.offs[mb, h] < T else 0
             for h in range(NH)] for mb in range(n_mb)]


# ------------------------------------------------------------------ reference and model
def _unit(x):
    x = x.double()
    n = x.norm(dim=-1, keepdim=True)
    return x / n.clamp_min(1e-12), n


def _normalize_bwd(G, xh, xn):
    return (G - xh * (xh * G).sum(-1, keepdim=True)) / xn


def _eval(c, model):
    """Forward and the pre-normalize gradients for a unit upstream gradient, in float64.
    model: round to bf16 what enters the second MFMA (see bf16_model)."""
    f64 = torch.float64
    B, T, NH, n_mb, n_max = geometry(c)
    tau, nk = c.tau, len(c.ks)
    yh, yn = _unit(c.y)
    th, tn = _unit(c.t)
    fixed = takes_fixed_shift(tau, c.logq is not None)[0]
    lse = torch.full((NH, n_mb, n_max), float("nan"), dtype=f64)
    pos, lse32 = lse.clone(), lse.clone()
    cnt = torch.zeros((NH, n_mb, n_max), dtype=torch.int64)
    rank, used = cnt.clone(), torch.zeros((NH, n_mb, n_max), dtype=torch.bool)
    live = used.clone()  # r < n
    pad_r = used.clone()
    stats = torch.zeros((NH, n_mb, ST_HITS + nk), dtype=f64)
    gsep = torch.zeros((B, T + 1, NH, DE), dtype=f64)
    gfus = torch.zeros_like(gsep) if (model and fixed) else None
    gin = torch.zeros((B, T, DE), dtype=f64)
    sdy = torch.zeros((B, T + 1, NH), dtype=f64)  # row_err's scales: w of the row's (mini-batch, head) ...
    sdt = torch.zeros((B, T), dtype=f64)          # ... and its sum over the heads that have the column
    gdy = torch.zeros((B, T + 1, NH), dtype=torch.int64)  # group ids: mb NH + h, and mb
    gdt = torch.zeros((B, T), dtype=torch.int64)
    loss = 0.0
    tau32 = torch.tensor(tau, dtype=torch.float32)
    for mb in range(n_mb):
        sl = slice(mb * c.mbs, min((mb + 1) * c.mbs, B))
        Bm = sl.stop - sl.start
        for h in range(NH):
            o = int(c.offs[mb, h])
            L = T - o
            stats[h, mb, ST_OFFSET] = o
            gdy[sl, :, h], gdt[sl] = mb * NH + h, mb
            if L <= 0:
                continue
            n = Bm * L
            out = yh[sl, :L, h].reshape(n, DE)
            inn = th[sl, o:].reshape(n, DE)
            pad = c.mask[sl, o:].reshape(n)
            seq = torch.arange(n) // L
            keep = seq[:, None] != seq[None, :]
            keep.fill_diagonal_(True)
            keep &= ~pad[None, :]
            keep &= ~pad[:, None]
            dots = out @ inn.T
            S = torch.where(keep, dots / tau, torch.tensor(-float("inf"), dtype=f64))
            cn = keep.sum(1)
            ps = S.diagonal().clone()
            rk = (S > ps[:, None]).sum(1)
            us = ~pad & (cn - 1 > 0)
            Sc = S
            S32 = torch.where(keep, dots.float() / tau32, torch.tensor(-float("inf")))
            if c.logq is not None:
                corr = c.logq[sl, o:].reshape(n)
                Sc = S + corr.double()[None, :]
                Sc.diagonal().copy_(ps)
                d32 = S32.diagonal().clone()
                S32 = S32 + corr[None, :]
                S32.diagonal().copy_(d32)
            ls = torch.logsumexp(Sc, 1)
            lse[h, mb, :n], pos[h, mb, :n], cnt[h, mb, :n], rank[h, mb, :n] = ls, ps, cn, rk
            lse32[h, mb, :n] = torch.logsumexp(S32, 1).double()
            used[h, mb, :n], live[h, mb, :n], pad_r[h, mb, :n] = us, True, pad
            U = int(us.sum())
            stats[h, mb, ST_USED] = stats[h, mb, ST_TOKENS] = U
            if U == 0:
                continue
            ce, neg, rku = (ls - ps)[us], (cn - 1)[us].double(), rk[us].double()
            mn = int(neg.min())
            stats[h, mb, ST_CE], stats[h, mb, ST_NEG], stats[h, mb, ST_MINNEG] = ce.mean(), neg.mean(), mn
            stats[h, mb, ST_RANK], stats[h, mb, ST_MEDIAN] = rku.mean(), rku.quantile(0.5)
            for q, k in enumerate(c.ks):
                stats[h, mb, ST_HITS + q] = float((rku < min(k, mn)).sum()) / U
            loss = loss + float(ce.mean()) / n_mb
            w = us.double() / (U * n_mb)
            sdy[sl, :L, h] = w.reshape(Bm, L)
            sdt[sl, o:] += (~pad).double().reshape(Bm, L) / (U * n_mb)
            P = torch.exp(Sc - torch.where(us, ls, torch.zeros_like(ls))[:, None]) * us.double()[:, None]
            dS = w[:, None] * P
            dS.diagonal().sub_(w)
            del P
            if model:
                dS = bf(dS)
            gin[sl, o:] += (dS.T @ out / tau).reshape(Bm, L, DE)
            gsep[sl, :L, h] = (dS @ inn / tau).reshape(Bm, L, DE)
            del dS
            if gfus is not None:
                p = torch.exp(S - 1.0 / tau) * us.double()[:, None]  # exp(-inf) = 0 on the excluded
                Z = p.sum(1)
                sc = torch.where(us, w / Z.clamp_min(1e-300), torch.zeros_like(w))
                gfus[sl, :L, h] = ((sc[:, None] * (bf(p) @ inn) - w[:, None] * inn) / tau).reshape(Bm, L, DE)
    sdy, sdt = sdy / yn[..., 0], sdt / tn[..., 0]  # dx = (G - x^ (x^ . G)) / |x|: the inputs' norms span 2^-3 .. 2^3
    return SimpleNamespace(lse=lse, pos=pos, cnt=cnt, rank=rank, used=used, live=live, pad=pad_r, lse32=lse32,
                           stats=stats, loss=loss, sdy=sdy, sdt=sdt, gdy=gdy, gdt=gdt, gsep=gsep, gfus=gfus, gin=gin, yh=yh, yn=yn, th=th, tn=tn)


def _grads(c, ev, kind, g, model):
    """dy, dt of the upstream gradient g from the pre-normalize gradients of _eval"""
    r = bf if model else (lambda x: x)
    dy = _normalize_bwd(ev.gfus if (kind == "fused" and model) else ev.gsep, ev.yh, ev.yn)
    if c.y.dtype == torch.bfloat16:
        dy = r(r(dy) * g) if kind == "fused" else r(dy * g)
    else:
        dy = dy * g
    dt = _normalize_bwd(ev.gin * g, ev.th, ev.tn)
    if c.t.dtype == torch.bfloat16:
        dt = r(dt)
    return dy, dt


def reference(c, g=None):
    """float64, no rounding anywhere (the module docstring's formulas).  Returns the per-row
    outputs, the statistics, the loss and dy / dt for the upstream gradient g (default c.g)."""
    ev = _eval(c, False)
    ev.dy, ev.dt = _grads(c, ev, "separate", c.g if g is None else g, False)
    return ev


KINDS = ("fused", "separate")


def bf16_model(c, g=None):
    """The same formulas with the bf16 roundings of the kernels (loss.hip).  Returns
    {kind: (dy, dt)}; the kinds differ in dy only.

    Both kinds:
      * dS = w (P - I) before dS^T . out, the columns pass (cl_bwd32_k<false, *>, cl_bwd32v_k and
        cl_bwd_k<false, *> pack the f32 dS to bf16 for the second MFMA; w carries 1 / (U n_mb) but
        not the upstream gradient, which scales the f32 result);
      * dt on store when the target is bf16 (normalize_bwd_store; rownorm_bwd on the per-head path).
    "separate" (cl_bwd32_k<true, *>, cl_bwd_k<true, *>: the ROWS pass after a separate forward,
    the running shift, logQ, the per-head backward, and the second backward of a retained graph):
      * dS before dS . in, as above;
      * dy on store when y is bf16, the upstream gradient already folded into the f32 value.
    "fused" (cl_fr32_k, cl_fr32v_k: the training forward at the fixed shift):
      * the unnormalised p = exp(S - 1/tau) before p . in; Z = sum p stays f32 and divides the
        f32 product, dOut = w (p . in / Z - in);
      * dy on store when y is bf16, for a unit upstream gradient, and again after cl_dyscale_k
        multiplied the stored value by g.
    Logits, lse, Z and the F.normalize arithmetic stay unrounded (f32 in the kernels).  An upper
    model of the rounding, not an emulation: the factor 4 of the bounds covers f32 accumulation
    order, exp2 / log approximations and f32 tau."""
    g = c.g if g is None else g
    ev = _eval(c, True)
    return {k: _grads(c, ev, k, g, True) for k in KINDS if k == "separate" or ev.gfus is not None}


def row_err(got, want, scale, floor=None):
    """Per-row error over the last axis, floored after the rows are put on one scale:
      |got - want| / max(|want|, FLOOR s_row max_rows(|want| / s)),
    as a tensor over the leading axes.  s is the row's scale (reference().sdy / .sdt): for dy row
    (b, t, h) the row weight w = 1 / (U n_mb) of its (mini-batch, head) over |y row|, for dt row (b, t)
    the sum of w over the heads that have the column (t >= o) over |t row|.  U differs by 100x to 1000x between the
    (mini-batch, head) pairs of one tensor (U = 2 beside 257, L = 1 beside 300), and a floor taken
    from the largest row of the whole tensor would sit above every row of the large pairs.  On the
    common scale |want| / s = |sum_c P in_c - in_r| is of order one in every pair, and the floor only
    catches the rows whose gradient cancels.  Rows with s = 0 have a zero reference (pads, t >= L,
    no negative): they are held to exact zeros by the tests and give 0 here."""
    got, want, scale = got.double(), want.double(), scale.double()
    wn = want.norm(dim=-1)
    live = scale > 0
    assert bool((wn[~live] == 0).all())
    if not bool(live.any()):
        raise ValueError("the reference is all zero: it is held exactly, not relatively")
    top = float((wn[live] / scale[live]).max())
    fl = (FLOOR if floor is None else floor) * top * scale
    err = (got - want).norm(dim=-1) / torch.maximum(wn, fl).clamp_min(1e-300)
    return torch.where(live, err, torch.zeros_like(err))


def typical_allowed(want, scale, group, bound, min_rows=1):
    """{group: the relative error the bound allows the median non-zero row of the group}:
    bound x max(1, floor / |row|).  A bound is only worth having while this stays near 0.1."""
    wn, scale = want.double().norm(dim=-1), scale.double()
    live = scale > 0
    top = float((wn[live] / scale[live]).max())
    out = {}
    for gid in torch.unique(group[live]).tolist():
        sel = live & (group == gid) & (wn > 0)
        if int(sel.sum()) >= min_rows:
            med = float((wn[sel] / scale[sel]).median())
            out[gid] = bound * max(1.0, FLOOR * top / med)
    return out


def worst(err):
    """(max, index) of an error tensor"""
    i = int(torch.argmax(err))
    return float(err.reshape(-1)[i]), tuple(int(x) for x in np.unravel_index(i, tuple(err.shape)))


@functools.lru_cache(maxsize=None)
def bounds(spec):
    """(case, reference, model maxima, bounds) of one Spec, computed once per session and never
    changed.  zero: the gradient tensors whose reference is exactly zero (held to exact zeros)."""
    c = make_case(spec)
    ref = reference(c)
    mod = bf16_model(c)
    zero = tuple(n for n in ("dy", "dt") if float(getattr(ref, n).abs().max()) == 0.0)
    mmax, bnd = {}, {}
    for kind, (dy, dt) in mod.items():
        for n, m in (("dy", dy), ("dt", dt)):
            if n in zero:
                assert float(m.abs().max()) == 0.0, (spec.name, n)
                continue
            mmax[n, kind] = float(row_err(m, getattr(ref, n), getattr(ref, "s" + n)).max())
            bnd[n, kind] = 4.0 * mmax[n, kind]
    u = ref.used
    if bool(u.any()):
        lse_floor = 2.0 ** -24 * float(ref.lse[u].abs().max())
        mmax["lse"] = max(float((ref.lse32[u] - ref.lse[u]).abs().max()), lse_floor)
    else:
        mmax["lse"] = 0.0
    bnd["lse"] = 8.0 * mmax["lse"]
    bnd["pos"] = float(np.spacing(np.float32(1.0 / c.tau)))
    bnd["ce"] = bnd["lse"] + bnd["pos"]
    bnd["loss"] = geometry(c)[2] * bnd["ce"]
    return SimpleNamespace(spec=spec, case=c, ref=ref, model_max=mmax, bound=bnd, zero=zero)


# ------------------------------------------------------------------ the case lists
def _split(m, k, cap):
    """m valid tokens over k sequences of at most cap, as even as possible"""
    out = [min(cap, m // k + (1 if i < m % k else 0)) for i in range(k)]
    assert sum(out) == m, (m, k, cap)
    return out


# a. valid counts: head 0 (offset 0) of mini-batch i has exactly M_VALUES[i] valid rows
M_VALUES = (1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 257)
_MV = tuple(v for m in M_VALUES for v in _split(m, 3, 100))
_MOFFS = tuple((0, 1 + i % 3) for i in range(len(M_VALUES)))
VALID = [
    Spec("m-left", 36, 100, 2, 3, 0.05, _MOFFS, valid=_MV, pads="left", seed=1),
    Spec("m-mixed", 36, 100, 2, 3, 0.05, _MOFFS, valid=_MV, pads="mixed", ydt="f32", seed=2),
]

# b. n itself at 64 k and 64 k +- 1 without pads (the full passes), B = mbs + 1: the ragged last
# mini-batch holds one sequence (no negative, no used row, zero gradients).  T = 1: L = 1
FULL_N = {63: (3, 21), 64: (4, 16), 65: (5, 13), 127: (127, 1), 128: (2, 64), 129: (3, 43), 193: (193, 1),
          257: (257, 1)}
FULL = [Spec(f"n{n}", mbs + 1, T, 1, mbs, 0.05, ((0,), (0,)), seed=10 + i)
        for i, (n, (mbs, T)) in enumerate(FULL_N.items())]

# c. sequence geometry: L = T - o in {300, 129, 63 | 100, 65, 2 | 1, 0, 300}: own-sequence blocks
# that start mid-tile and cross tile edges, L > 128 (a whole 64-column tile of the row's own
# sequence), a head with offset >= T in the last mini-batch; sequence 1 all pad, 2 and 3 with one
# and two valid tokens (min negatives below the smallest k), random left pads elsewhere
GEO_L = (300, 129, 63, 100, 65, 2, 1, 0, 300)
_GEO_VALID = (300, 0, 1, 2, 251, 300, 17, 180, 300, 299, 150, 64)
GEOMETRY = [Spec("geo", 12, 300, 3, 4, 0.05, ((0, 171, 237), (200, 235, 298), (299, 300, 0)), valid=_GEO_VALID, seed=20)]

# d. many short sequences: about 21 sequence boundaries in a 64-column tile; 40 sequences a mini-batch
SHORT = [
    Spec("mbs130-T3", 261, 3, 2, 130, 0.05, ((0, 1), (0, 2), (1, 0)), seed=30),
    Spec("mbs40-T8", 80, 8, 2, 40, 0.05, ((0, 3), (2, 7)), valid=tuple((5 * i + 3) % 9 for i in range(80)),
         pads="mixed", seed=31),
]

# e. degenerate: one sequence per mini-batch throughout: the loss is the constant 0
ONE_SEQ = [Spec("mbs1", 3, 20, 2, 1, 0.05, ((0, 2), (0, 3), (1, 5)), seed=40),
           Spec("mbs1-run", 3, 20, 2, 1, 0.01, ((0, 2), (0, 3), (1, 5)), seed=40)]

# f. statistics workspace: n = 2,080 puts rows in a second CL_SROWS block and n_max = 2,112 > n
# (with a ragged one-sequence mini-batch); n = 4,096 = 32 x 128 has n_max == n
STATS_WS = [
    Spec("n2080", 33, 65, 2, 32, 0.05, ((0, 2), (0, 1)), valid=tuple(65 - (7 * i) % 40 for i in range(33)), seed=50),
    Spec("n4096", 32, 128, 1, 32, 0.05, ((0,),), valid=tuple(128 - (11 * i) % 90 for i in range(32)), seed=51),
]

# g. softmax range (make_case, adv): tau = 0.025 is the last fixed-shift value (every p of an (a)
# row but the positive's is e^-80), the f32 below it and 0.01 (logits +-100) take the running shift;
# 0.07 is a fixed-shift temperature whose 1 / tau is inexact in f32 (the ties of (d))
_ADV_OFFS = ((0, 3), (0, 3), (0, 2))
RANGE = [Spec(f"adv-{nm}", 9, 50, 2, 3, tau, _ADV_OFFS, adv=True, seed=60)
         for nm, tau in (("tau0.025", TAU_LAST_FIXED), ("below0.025", TAU_FIRST_RUNNING), ("tau0.01", 0.01), ("tau0.07", 0.07))]

# h. logQ corrections over +-6.44 on pads and non-pads
LOGQ = [Spec(f"logq-tau{tau}", 7, 50, 2, 3, tau, ((0, 4), (1, 9), (0, 2)), valid=(50, 31, 0, 50, 1, 44, 50), logq=True,
             seed=70) for tau in (0.05, 0.01)]

# i. dtypes, heads and upstream gradients
_DT = dict(B=7, T=50, mbs=3, tau=0.05, valid=(50, 31, 0, 50, 2, 44, 50))
DTYPES = [Spec(f"y{yd}-t{td}", NH=NH, offs=tuple(tuple(range(i, i + NH)) for i in range(3)), ydt=yd, tdt=td,
               seed=80 + NH, **_DT)
          for NH, yd, td in ((1, "bf16", "f32"), (2, "bf16", "bf16"), (3, "f32", "f32"), (2, "f32", "bf16"))]
HEADS6 = [Spec("nh6", 8, 40, 6, 4, 0.05, ((0, 1, 5, 11, 24, 30), (0, 2, 6, 12, 20, 39)), tdt="bf16",
               valid=(40, 12, 0, 33, 40, 40, 1, 25), seed=86)]
UPSTREAM = [Spec(f"g{g}-y{yd}", NH=2, offs=((0, 3), (1, 2), (0, 5)), ydt=yd, g=g, seed=90, **_DT)
            for g, yd in ((2.5, "bf16"), (-0.75, "bf16"), (2.5, "f32"))]
RETAIN = (Spec("retain", NH=2, offs=((0, 3), (1, 2), (0, 5)), g=1.0, seed=91, **_DT), 2.5)  # g1, then g2

ALL = VALID + FULL + GEOMETRY + SHORT + ONE_SEQ + STATS_WS + RANGE + LOGQ + DTYPES + HEADS6 + UPSTREAM + [RETAIN[0]]
NO_USED_ROW = tuple(s.name for s in ONE_SEQ)  # the only cases meant to have no used row at all
BY_NAME = {s.name: s for s in ALL}
assert len(BY_NAME) == len(ALL)
