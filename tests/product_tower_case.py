"""Inputs, float64 references and per-element bounds for lthm_product_tower_fwd (csrc/towers.hip).

Nothing is imported from the package under test.  The reference restates ProductTower.forward
(models/lthm/sequence/product_tower.py:43-62) and CosineVectorEmbedding.forward
(commons/transformers/layers.py:462-471) in float64 from the raw inputs:

    nrm  = |x|                         mask = nrm < threshold  or  id == 0
    xn   = x / max(nrm, 1e-12)         xn2  = xn / max(|xn|, 1e-12)   (cve_only: xn2 = xn)
    z    = xn2 . P[:, p]               bucket = #{q : grid[q] < z}    (bucketize, right = False)
    row  = row_off + (nb + 1) p + bucket
    hbin = clamp(floor(nrm nbins), 0, nbins - 1)
    emb  = b + W xn + sum_p Tab[row_p] + Hist[hbin],  zero where masked

with the inputs as the kernel reads them: x in its own type (f32 or bf16), the tables as given
(on the MFMA path they are bf16, and 0/1 times a bf16 is exact), 1e-12 as its float32 image
(F.normalize clamps float32 tensors at that value).

u = 2^-24 is the relative error of one float32 operation rounded to nearest.

Radius of z (the kernels: two normalisations, then Din sequential FMAs).  The first
normalisation scales every element by the same computed 1 / max(nrm, 1e-12), and a common factor
drops out of the second normalisation, so of the first only the Din division roundings remain:
xn_i = x_i / |x| (1 + d_i) c, |d_i| <= u.  The second computes ss2 = sum xn_i^2 (Din products
and Din - 1 additions of positive terms: relative error <= Din u), its square root (halves that,
adds u) and one division per element (u); the norm of the perturbed vector itself lies within u
of c.  Hence |xn2_i - x_i / |x|| <= (u + u + (Din / 2 + 1) u + u) |x_i| / |x| <= (Din / 2 + 4) u
|xn2_i|; a tree sum (the per-token kernel's wave reduction) has fewer roundings.  cve_only has
one normalisation: (Din / 2 + 2) u.  The Din sequential FMAs round Din partial sums:
Din u sum |xn2_i P_ip|.  Together
    |z_kernel - z| <= c(Din) u sum_i |xn2_i P_ip|,   c(Din) = Din + Din / 2 + 4 + 2 = 1.5 Din + 6,
the last 2 covering every second-order term ((2 Din u)^2 << u for Din <= 256).  A pair (token,
projection) whose z lies within that radius of a grid value is AMBIGUOUS: the kernel may return
either bucket next to that grid value and nothing else.  Everywhere else the row is exact.

Radius of nrm: ss = sum x_i^2 (<= Din u), square root (Din / 2 + 1) u: r_n = (Din / 2 + 1) u nrm.
The mask compares nrm with the threshold (ambiguous within r_n); the histogram bin takes
floor(nrm nbins), one more rounding: ambiguous where nrm nbins lies within (Din / 2 + 2) u nrm
nbins of an integer in 1 .. nbins - 1.  The cases' seeds are chosen so that NO random token is
ambiguous for either, and at most 1e-3 of a case's pairs are ambiguous (checked on the CPU).

Planted tokens x = a e_0, a a power of two (or the threshold): nrm = a, xn = xn2 = e_0 and
z = P[0, p] with every operation exact, so they carry radius 0.  For some projections P[0, p] is
set to one of the module's grid values: the tie falls in the lower bucket (a <= for < moves it).
a = threshold: not masked; a = threshold - 1 ulp of x's type: masked (a^2 rounds to a float32
whose correctly rounded root is a again, and a / a = 1: exact like the others); a = 0.5: bin nbins // 2; a = 1, 2: the last bin; an
all-zero x (masked, xn = 0); tokens with id 0 (rows 0xffff, emb 0, mask 1); and a token
2^-50 e_1 whose first normalisation leaves |xn| = 2^-50 / 1e-12: only the second one makes it a
unit vector (seen where the threshold is below 2^-50, and in cve_only, which must NOT apply it).

Continuous outputs, per element.  For a float32 value v with |v - ref| <= e, the stored output
rn(v) satisfies |rn(v) - ref| <= e + half_ulp_out(|ref| + e): one output rounding at the value
it is applied to.  That form also admits the neighbouring bf16 value exactly where ref lies
within e of a rounding boundary.
  xn_out (bf16):  e = (Din / 2 + 2) u |xn|   (ss, root, division).
  emb_out:  e = T u S + (Din / 2 + 2) u M + split,  S = |b| + M + sum |Tab rows| + |Hist row|,
      M = sum_i |xn_i W_oi|, T the number of summed terms (each addition rounds once):
      per token  T = 1 + Din + slots + modules + 1;   MFMA  T = 3 Din + slots + 1,
      the second term the error of xn itself, and on the MFMA path
      split = (2^-14 + 2^-15 + 2^-20) M:  each operand v = hi + lo + r with hi the top 16 bits
      (|v - hi| < 2^-7 |v|), lo = bf16(v - hi) (|r| <= 2^-9 2^-7 |v| = 2^-16 |v|); the kernel sums
      hi hi + hi lo + lo hi, dropping lo lo (<= 2^-14 |x w|) and the two r terms (<= 2^-15 |x w|).
  A masked token's emb is exactly 0.
"""
import math
from collections import namedtuple
from types import SimpleNamespace

import torch

U = 2.0 ** -24
EPS = float(torch.tensor(1e-12, dtype=torch.float32))
PAD_VALUE = 3.0e4  # table rows at and beyond R: large and finite

# mods: ((n_proj, num_bins), ...); tab: "bf16", "f32" or "f32img" (float32 storage of bf16 values: the
# same numbers as a bf16 case, on the per-token kernel); plan: what lthm_product_tower_plan must say
Spec = namedtuple("Spec", "name n Din Dout mods nbins xbf tab embf32 bias cve_only thr rows_out seed plan")
Plan = namedtuple("Plan", "path dm full nf dma nslice nslab opl", defaults=(0, 0, 0, 0, 1, 0, 0))


def _mf(dm, full, nf, dma, nslab, nslice=1):
    return Plan("mfma", dm, full, nf, dma, nslice, nslab, {1: 1, 2: 1, 4: 1, 8: 2, 16: 4}[nf] if nslice == 1 else 8)


def _tk(opl, nslab, nslice=1):
    return Plan("token", 0, 0, 0, 0, nslice, nslab, opl)


def _S(name, n, Din, Dout, mods, nbins, plan, xbf=False, tab="bf16", embf32=False, bias=True, cve_only=False,
       thr=0.0625, rows_out=True, seed=0):
    return Spec(name, n, Din, Dout, tuple(mods), nbins, xbf, tab, embf32, bias, cve_only, thr, rows_out, seed, plan)


TINY = 2.0 ** -60  # a threshold below the 2^-50 token: the second normalisation becomes visible

MFMA_SPECS = [
    # rows DM 32 full, NF 16 with the ring, 9 slabs, R = 262 (not a multiple of 32), three chunks of rows
    _S("ring16_s9", 513, 32, 256, ((5, 32), (1, 20), (3, 1), (6, 8)), 16, _mf(32, 1, 16, 1, 9)),
    _S("ring16_s1", 129, 20, 256, ((3, 4),), 8, _mf(32, 0, 16, 1, 1), xbf=True),
    _S("ring16_s2", 128, 28, 256, ((2, 20), (1, 1)), 0, _mf(32, 0, 16, 1, 2), bias=False),
    _S("ring8_s3", 257, 64, 128, ((5, 16),), 11, _mf(64, 1, 8, 1, 3), xbf=True),  # R = 96
    _S("ring8_s4", 127, 36, 128, ((6, 16),), 10, _mf(64, 0, 8, 1, 4)),            # Din 36: the mapper's 4-wide k-tail
    _S("ring8_s5", 255, 60, 128, ((7, 20),), 4, _mf(64, 0, 8, 1, 5), xbf=True, bias=False),
    _S("reg16_s2", 256, 16, 256, ((2, 20),), 8, _mf(32, 0, 16, 0, 2)),
    _S("reg8_s3", 129, 8, 128, ((4, 16),), 5, _mf(32, 0, 8, 0, 3)),
    _S("nf1_n1", 1, 4, 16, ((1, 1),), 0, _mf(32, 0, 1, 0, 1)),
    _S("nf2_tiny", 257, 12, 32, ((3, 32), (2, 5)), 0, _mf(32, 0, 2, 0, 4), thr=TINY),
    # 256 projections: every thread of the rows kernel owns one; a masked token in all 16 tile positions
    _S("nf4_p256", 400, 32, 64, ((200, 7), (56, 1)), 32, _mf(32, 1, 4, 0, 55), xbf=True),
    _S("slices2", 129, 32, 512, ((4, 20), (2, 32)), 16, _mf(32, 1, 16, 1, 6, 2)),
]
TOKEN_SPECS = [
    _S("opl1_f32", 70, 200, 24, ((5, 20), (3, 1)), 8, _tk(1, 4), tab="f32", embf32=True),
    _S("opl2_p70", 65, 37, 100, ((70, 4),), 0, _tk(2, 11), xbf=True, tab="f32", thr=TINY),
    # 40 bins: past the rows kernel's 32, an otherwise MFMA-eligible descriptor
    _S("opl4_nb40", 129, 32, 256, ((5, 40), (1, 20)), 16, _tk(4, 8)),
    _S("opl8_384", 33, 30, 384, ((4, 10),), 4, _tk(8, 2), xbf=True, embf32=True, bias=False),
    _S("cve_f32", 100, 32, 64, ((16, 20),), 0, _tk(1, 11), tab="f32", embf32=True, bias=False, cve_only=True),
    _S("cve_bf16", 50, 37, 128, ((4, 20),), 0, _tk(2, 3), xbf=True, bias=False, cve_only=True, rows_out=False),
    # the numbers of ring16_s9 with float32 table storage: the same descriptor on the per-token kernel
    _S("cross_f32img", 513, 32, 256, ((5, 32), (1, 20), (3, 1), (6, 8)), 16, _tk(4, 9), tab="f32img"),
]
SPECS = MFMA_SPECS + TOKEN_SPECS
CROSS = ("ring16_s9", "cross_f32img")
BY_NAME = {s.name: s for s in SPECS}


def bf(t):
    """float64 -> nearest bf16 (ties to even), as float64; no double rounding through float32"""
    t = t.double()
    m, e = torch.frexp(t)
    return torch.ldexp(torch.round(m * 256.0), e - 8)  # torch.round: half to even


def half_ulp(v, f32):
    """half an ulp of the output type at |v| (float64 tensor)"""
    _, e = torch.frexp(v.abs().clamp_min(2.0 ** -120))
    return torch.ldexp(torch.ones_like(v), e - (25 if f32 else 9))


def grid_of(nb):
    res = 2.0 / float(nb)  # layers.py:450-451
    return torch.linspace(-1.0, 1.0, steps=nb + 1)[:-1] + 0.5 * res


PLANTS = ("tie", "thr", "below", "half", "one", "two", "zero", "id0", "tiny", "tie2")


def make_case(spec):
    g = torch.Generator().manual_seed(1000 * (SPECS.index(BY_NAME[spec.name]) + 1 if spec.name in BY_NAME else 99)
                                      + spec.seed)
    if spec.name == "cross_f32img":  # the very inputs of its MFMA twin
        c = make_case(BY_NAME["ring16_s9"])
        c.spec = spec
        c.tab = c.tab.float()
        return c
    n, Din, Dout = spec.n, spec.Din, spec.Dout
    rnd = lambda *s: torch.randn(*s, generator=g)
    c = SimpleNamespace(spec=spec)
    c.proj, c.grid, c.row_off = [], [], []
    ro = 0
    for (np_, nb) in spec.mods:
        P = torch.nn.functional.normalize(rnd(Din, np_), p=2.0, dim=0)
        gr = grid_of(nb)
        for p in range(min(np_, 3)):  # the ties of the planted tokens
            P[0, p] = gr[(5 * p + 1) % nb]
        c.proj.append(P.contiguous())
        c.grid.append(gr.contiguous())
        c.row_off.append(ro)
        ro += (nb + 1) * np_
    c.cve_rows = ro
    c.R = ro + spec.nbins
    c.total = sum(m[0] for m in spec.mods) + (1 if spec.nbins else 0)
    R32 = (c.R + 31) // 32 * 32
    tab = (0.25 * rnd(R32 + 1, Dout)).bfloat16().float() if spec.tab != "f32" else 0.25 * rnd(R32 + 1, Dout)
    tab[c.R:] = PAD_VALUE
    c.tab = tab.bfloat16() if spec.tab == "bf16" else tab
    c.w_map = (rnd(Dout, Din) / math.sqrt(Din)).contiguous()
    c.b_map = 0.5 * rnd(Dout) if spec.bias else None
    radius = 0.1 + 0.85 * torch.rand(n, 1, generator=g)
    x = torch.nn.functional.normalize(rnd(n, Din), dim=1) * radius
    ids = torch.randint(1, 1 << 40, (n,), generator=g)
    t = torch.arange(n)
    ids[t % 17 == 3] = 0
    # planted tokens, spread over the token range; a case too short for all of them takes the first
    kinds = PLANTS[:n] if n < 2 * len(PLANTS) else PLANTS
    c.plant = {}
    ulp = 2.0 ** -8 if spec.xbf else 2.0 ** -24
    for k, kind in enumerate(kinds):
        pos = (k * n) // len(kinds) + (1 if n >= 2 * len(kinds) else 0)
        a = {"tie": 0.25, "thr": spec.thr, "below": spec.thr * (1.0 - ulp), "half": 0.5, "one": 1.0, "two": 2.0,
             "zero": 0.0, "tiny": 2.0 ** -50, "tie2": 4.0}.get(kind)
        ids[pos] = 0 if kind == "id0" else 12345 + k
        if kind != "id0":
            x[pos] = 0.0
            x[pos, 1 if a < 1e-6 and a > 0 else 0] = a  # below 1e-12: off the axis of the planted ties
        c.plant[kind] = pos
    # exact: z is exact (radius 0); nexact: nrm is exact.  Below 1e-12 the first normalisation
    # divides by 1e-12 and rounds, so a threshold token of the TINY cases has an exact norm only
    c.exact = torch.zeros(n, dtype=torch.bool)
    c.nexact = torch.zeros(n, dtype=torch.bool)
    for kind, pos in c.plant.items():
        if kind not in ("id0", "tiny") and not (kind in ("thr", "below") and spec.thr < 1e-6):
            c.exact[pos] = True
        if kind != "id0":
            c.nexact[pos] = True
    c.x = x.bfloat16() if spec.xbf else x.contiguous()
    c.ids = None if spec.cve_only else ids
    return c


def reference(c):
    """The float64 restatement and its decision radii."""
    s = c.spec
    Din = s.Din
    x = c.x.double()
    r = SimpleNamespace()
    r.nrm = x.pow(2).sum(1).sqrt()
    r.mask = torch.zeros(s.n, dtype=torch.bool) if s.cve_only else (r.nrm < s.thr) | (c.ids == 0)
    r.xn = x / r.nrm.clamp_min(EPS)[:, None]
    r.xn2 = r.xn if s.cve_only else r.xn / r.xn.pow(2).sum(1).sqrt().clamp_min(EPS)[:, None]
    cz = (0.5 * Din + 2 + Din + 2) if s.cve_only else (1.5 * Din + 6)
    zs, rads, lo, hi, base = [], [], [], [], []
    for j, (np_, nb) in enumerate(s.mods):
        P, gr = c.proj[j].double(), c.grid[j].double()
        z = r.xn2 @ P
        rad = cz * U * (r.xn2.abs() @ P.abs())
        rad[c.exact] = 0.0
        zs.append(z)
        rads.append(rad)
        lo.append((gr[None, None, :] < (z - rad)[:, :, None]).sum(-1))
        hi.append((gr[None, None, :] < (z + rad)[:, :, None]).sum(-1))
        base.append(c.row_off[j] + (nb + 1) * torch.arange(np_)[None, :].expand(s.n, -1))
    cat = lambda l: torch.cat(l, 1) if l else torch.zeros(s.n, 0, dtype=torch.int64)
    r.z, r.zrad, r.lo, r.hi, r.base = cat(zs), cat(rads), cat(lo), cat(hi), cat(base)
    r.bucket = cat([(c.grid[j].double()[None, None, :] < zs[j][:, :, None]).sum(-1) for j in range(len(s.mods))])
    r.amb = r.lo != r.hi
    rn = (0.5 * Din + 1) * U * r.nrm
    rn[c.nexact] = 0.0
    r.mask_amb = torch.zeros(s.n, dtype=torch.bool) if s.cve_only else ((r.nrm - s.thr).abs() <= rn) & (rn > 0)
    if s.nbins:
        f = r.nrm * s.nbins
        r.hbin = torch.floor(f).clamp(0, s.nbins - 1).long()
        rf = rn * s.nbins + U * f
        near = torch.round(f)
        r.hist_amb = ((f - near).abs() <= rf) & (rn > 0) & (near >= 1) & (near <= s.nbins - 1)
    else:
        r.hbin, r.hist_amb = None, torch.zeros(s.n, dtype=torch.bool)
    return r


def ref_rows(c, r, bucket=None):
    """[n, total] rows of the reference (or of another bucket choice), 0xffff where masked"""
    rows = r.base + (r.bucket if bucket is None else bucket)
    if c.spec.nbins:
        rows = torch.cat([rows, (c.cve_rows + r.hbin)[:, None]], 1)
    return torch.where(r.mask[:, None], torch.full_like(rows, 0xffff), rows)


def ambiguity(c, r):
    """(share of ambiguous pairs among the unmasked tokens' pairs, mask-ambiguous, histogram-ambiguous tokens)"""
    pairs = r.amb[~r.mask]
    return (float(pairs.double().mean()) if pairs.numel() else 0.0), int(r.mask_amb.sum()), int(r.hist_amb.sum())


def inputs_ok(c, r):
    share, ma, ha = ambiguity(c, r)
    return share <= 1e-3 and ma == 0 and ha == 0 and (c.spec.rows_out or share == 0.0)


def check_discrete(c, r, rows, mask):
    """rows [n, total] (any integer type, or None), mask [n] (or None) as the kernel wrote them.
    Returns (problem or None, the rows the embedding reference must use)."""
    s = c.spec
    want = ref_rows(c, r)
    if mask is not None:
        bad = torch.nonzero(mask.bool() != r.mask).view(-1)
        if bad.numel():
            return f"mask differs at tokens {bad[:5].tolist()}", want
    if rows is None:
        return None, want
    rows = rows.long() & 0xffff
    if tuple(rows.shape) != tuple(want.shape):
        return f"rows shape {tuple(rows.shape)}", want
    npj = r.base.shape[1]
    ok = rows == want
    b = rows[:, :npj] - r.base
    ok[:, :npj] |= r.amb & ~r.mask[:, None] & (b >= r.lo) & (b <= r.hi)
    bad = torch.nonzero(~ok)
    if bad.numel():
        t, p = bad[0].tolist()
        return f"row of token {t} slot {p}: {int(rows[t, p])}, reference {int(want[t, p])} ({bad.shape[0]} differ)", want
    return None, rows


def terms(c, r, rows):
    """The pieces of emb in float64 from the given rows (masked tokens' rows are ignored)."""
    s = c.spec
    tab = c.tab.double()
    safe = torch.where(r.mask[:, None], torch.zeros_like(rows), rows)
    t = SimpleNamespace()
    npj = r.base.shape[1]
    g = tab[safe[:, :npj]]                       # [n, nproj, Dout]
    t.bag, t.bag_abs = g.sum(1), g.abs().sum(1)
    t.hist = tab[safe[:, npj]] if s.nbins else torch.zeros(s.n, s.Dout, dtype=torch.float64)
    if s.cve_only:
        t.map = t.map_abs = torch.zeros(s.n, s.Dout, dtype=torch.float64)
    else:
        W = c.w_map.double()
        t.map, t.map_abs = r.xn @ W.t(), r.xn.abs() @ W.abs().t()
    t.bias = c.b_map.double()[None, :].expand(s.n, -1) if c.b_map is not None and not s.cve_only else torch.zeros(s.n, s.Dout, dtype=torch.float64)
    return t


def emb_reference(c, r, rows, t=None):
    """(emb float64, per-element bound) for the rows the kernel used (check_discrete's second value)"""
    s = c.spec
    t = t or terms(c, r, rows)
    ref = t.bias + t.map + t.bag + t.hist
    S = t.bias.abs() + t.map_abs + t.bag_abs + t.hist.abs()
    slots = c.total
    if s.plan.path == "mfma":
        T, split = 3 * s.Din + slots + 1, (2.0 ** -14 + 2.0 ** -15 + 2.0 ** -20) * t.map_abs
    else:
        T, split = 1 + s.Din + slots + len(s.mods) + 1, 0.0
    e = T * U * S + (0.5 * s.Din + 2) * U * t.map_abs + split
    bound = e + half_ulp(ref.abs() + e, s.embf32)
    ref = torch.where(r.mask[:, None], torch.zeros_like(ref), ref)
    bound = torch.where(r.mask[:, None], torch.zeros_like(bound), bound)
    return ref, bound


def xn_reference(c, r):
    e = (0.5 * c.spec.Din + 2) * U * r.xn.abs()
    return r.xn, torch.where(r.xn == 0, torch.zeros_like(e), e + half_ulp(r.xn.abs() + e, False))


def ratio(got, ref, bound):
    """max |got - ref| / bound; where the bound is 0 the value must be equal"""
    d = (got.double() - ref).abs()
    if not torch.isfinite(got.double()).all():
        return float("inf")
    q = torch.where(bound > 0, d / bound.clamp_min(1e-300), torch.where(d > 0, torch.full_like(d, float("inf")), torch.zeros_like(d)))
    return float(q.max()) if q.numel() else 0.0


# ------------------------------------------------------------------ a float32 evaluation in the kernels' order
def _f32(t):
    return t.to(torch.float32)


def _fma(a, b, acc):
    """float32 fma: the product of two float32 is exact in float64"""
    return _f32(a.double() * b.double() + acc.double())


def _seq_sum(terms_, order):
    """float32 sum of a list of tensors: 0 ascending, 1 descending, 2 pairwise"""
    if order == 1:
        terms_ = terms_[::-1]
    if order == 2:
        while len(terms_) > 1:
            terms_ = [terms_[i] + terms_[i + 1] if i + 1 < len(terms_) else terms_[i] for i in range(0, len(terms_), 2)]
        return terms_[0]
    acc = terms_[0]
    for v in terms_[1:]:
        acc = acc + v
    return acc


def trunc16(v):
    return (v.contiguous().view(torch.int32) & -65536).view(torch.float32)


def evaluate_f32(c, order=0):
    """What a correct kernel may return: float32 arithmetic in the kernel's order (order 0), or with
    the projection sum and the bag sum descending (1) or pairwise (2).  Returns rows, mask, xn (bf16
    values), emb (values of the output type), all as the kernel would store them."""
    s = c.spec
    n, Din = s.n, s.Din
    x = _f32(c.x)
    eps = torch.tensor(EPS, dtype=torch.float32)
    ss = _seq_sum([x[:, i] * x[:, i] for i in range(Din)], 0)
    nrm = ss.sqrt()
    mask = torch.zeros(n, dtype=torch.bool) if s.cve_only else (nrm < s.thr) | (c.ids == 0)
    xn = x / torch.maximum(nrm, eps)[:, None]
    if s.cve_only:
        xn2 = xn
    else:
        ss2 = _seq_sum([xn[:, i] * xn[:, i] for i in range(Din)], 0)
        xn2 = xn / torch.maximum(ss2.sqrt(), eps)[:, None]
    rows = []
    for j, (np_, nb) in enumerate(s.mods):
        P = c.proj[j]
        if order == 2:
            z = _seq_sum([xn2[:, i:i + 1] * P[i][None, :] for i in range(Din)], 2)
        else:
            z = torch.zeros(n, np_)
            for i in (range(Din) if order == 0 else reversed(range(Din))):
                z = _fma(xn2[:, i:i + 1], P[i][None, :], z)
        bk = (c.grid[j][None, None, :] < z[:, :, None]).sum(-1)
        rows.append(c.row_off[j] + (nb + 1) * torch.arange(np_)[None, :] + bk)
    if s.nbins:
        hb = torch.floor(nrm * float(s.nbins)).clamp(0, s.nbins - 1).long()
        rows.append((c.cve_rows + hb)[:, None])
    rows = torch.cat(rows, 1)
    tab = _f32(c.tab)
    npj = rows.shape[1] - (1 if s.nbins else 0)
    if s.plan.path == "mfma":
        W = c.w_map
        xh, wh = trunc16(xn), trunc16(W)
        xl, wl = _f32(bf((xn - xh).double())), _f32(bf((W - wh).double()))
        acc = torch.zeros(n, s.Dout)
        for i in range(Din):
            for a, b in ((xh, wh), (xh, wl), (xl, wh)):
                acc = acc + a[:, i:i + 1] * b[:, i][None, :]  # a bf16 x bf16 product is exact in float32
        # the one-hot GEMM adds the table rows in ascending row order: slots are in that order already
        acc = acc + _seq_sum([tab[rows[:, p]] for p in range(rows.shape[1])], order)
        if c.b_map is not None:
            acc = acc + c.b_map[None, :]
    else:
        acc = torch.zeros(n, s.Dout)
        if not s.cve_only:
            acc = acc + (c.b_map[None, :] if c.b_map is not None else 0.0)
            for i in range(Din):
                acc = _fma(xn[:, i:i + 1], c.w_map[:, i][None, :], acc)
        p0 = 0
        for (np_, nb) in s.mods:
            acc = acc + _seq_sum([torch.zeros(n, s.Dout)] + [tab[rows[:, p0 + p]] for p in range(np_)], order)
            p0 += np_
        if s.nbins:
            acc = acc + tab[rows[:, npj]]
    acc = torch.where(mask[:, None], torch.zeros_like(acc), acc)
    emb = acc.double() if s.embf32 else bf(acc.double())
    rows = torch.where(mask[:, None], torch.full_like(rows, 0xffff), rows)
    return SimpleNamespace(rows=rows, mask=mask, xn=bf(xn.double()), emb=emb)


# ------------------------------------------------------------------ the descriptor, as ProductTowerFn fills it
def fill_desc(d, c, ptr):
    """Fill a lthm_ptower_desc from a case.  ptr: name -> address (or None) of ids, x, w_map, b_map, proj, grids,
    tables, emb_out, rows_out, xn_out, mask_out; the plan reads only whether they are null."""
    s = c.spec
    d.ids, d.x, d.x_dtype, d.Din, d.n, d.Dout = ptr["ids"], ptr["x"], int(s.xbf), s.Din, s.n, s.Dout
    d.n_mod = len(s.mods)
    d.w_map, d.b_map, d.proj, d.grids = ptr["w_map"], ptr["b_map"], ptr["proj"], ptr["grids"]
    row_bytes = s.Dout * (2 if s.tab == "bf16" else 4)
    d.tables, d.tab_dtype = ptr["tables"], int(s.tab == "bf16")
    d.hist = ptr["tables"] + c.cve_rows * row_bytes if s.nbins else None
    d.proj_total, d.grid_total = sum(P.numel() for P in c.proj), sum(g.numel() for g in c.grid)
    d.cve_rows, d.norm_bins, d.norm_threshold = c.cve_rows, s.nbins, s.thr
    d.cve_only, d.emb_dtype = int(s.cve_only), int(not s.embf32)
    po = go = 0
    for j, (np_, nb) in enumerate(s.mods):
        d.mod_nproj[j], d.mod_nbins[j], d.mod_row_off[j] = np_, nb, c.row_off[j]
        d.mod_proj_off[j], d.mod_grid_off[j] = po, go
        po += c.proj[j].numel()
        go += c.grid[j].numel()
    d.emb_out, d.rows_out, d.xn_out, d.mask_out = ptr["emb_out"], ptr["rows_out"], ptr["xn_out"], ptr["mask_out"]
    return d


def host_ptrs(c):
    """Stand-in addresses for the plan on a host without a GPU: non-null exactly where the case gives a tensor"""
    s = c.spec
    tower = None if s.cve_only else 64
    return dict(ids=tower, x=64, w_map=tower, b_map=64 if c.b_map is not None else None, proj=64, grids=64, tables=64,
                emb_out=64, rows_out=64 if s.rows_out else None, xn_out=tower, mask_out=tower)
