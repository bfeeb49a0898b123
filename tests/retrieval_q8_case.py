"""CPU restatement of the e4m3 catalogue (csrc/retrieve.hip: retr_q8_quant_k, retr_q8_topk_k,
retr_rescore_k) and the checkers the host and GPU tests share.

Quantiser: a = max |x_k| = m 2^p with m in [0.5, 1) (torch.frexp); e = 9 - p if m <= 0.875 else 8 - p,
clamped to [-64, 64], 0 for a = 0; codes = (x.float() * 2.0**e).to(torch.float8_e4m3fn); scale = 2^-e.
Approximate score: the fp64 dot of the dequantised codes (every product and sum of them is exact in
fp64: codes are 4-bit significands times powers of two).  Lists are ordered by numpy.lexsort on
(row, -score): score descending, row ascending.
"""
import numpy as np
import torch
import torch.nn.functional as F

D = 128
EPS = 1e-5
_CACHE = {}


def quant_exponent(x_bf):
    """int32 [N]: the exponent e of every bf16 row."""
    a = x_bf.float().abs().amax(dim=1)
    m, p = torch.frexp(a)
    e = torch.where(m <= 0.875, 9 - p, 8 - p).clamp(-64, 64)
    return torch.where(a == 0, torch.zeros_like(e), e).to(torch.int32)


def quantize_ref(x_bf):
    """(codes uint8 [N, 128], scale f32 [N], e int32 [N]) of bf16 rows."""
    assert x_bf.dtype == torch.bfloat16 and x_bf.dim() == 2
    e = quant_exponent(x_bf)
    up = torch.ldexp(torch.ones(e.shape, dtype=torch.float32), e)
    codes = (x_bf.float() * up[:, None]).to(torch.float8_e4m3fn)
    scale = torch.ldexp(torch.ones(e.shape, dtype=torch.float32), -e)
    return codes.view(torch.uint8), scale, e


def dequant(codes_u8, scale):
    return codes_u8.view(torch.float8_e4m3fn).double() * scale.double()[:, None]


def approx_scores(q_bf, items_bf):
    """fp64 [Q, N]: the approximate score of the bf16 query rows against the bf16 catalogue rows."""
    cq, sq, _ = quantize_ref(q_bf)
    ci, si, _ = quantize_ref(items_bf)
    return (dequant(cq, sq) @ dequant(ci, si).T).numpy()


def exact_scores(q_bf, items_bf):
    return (q_bf.double() @ items_bf.double().T).numpy()


def mask_rows(s, excl):
    """s with -inf at every (q, row) the int [Q, X] lists name (entries outside [0, N) ignored)."""
    s = s.copy()
    if excl is not None:
        N = s.shape[1]
        for i, lst in enumerate(np.asarray(excl)):
            ok = lst[(lst >= 0) & (lst < N)]
            s[i, ok] = -np.inf
    return s


def first_m(s, M):
    """(scores f32 [Q, M], rows int32 [Q, M]): the M first of s [Q, N] under (score descending, row
    ascending), -inf entries being no rows; then (-inf, -1)."""
    Q, N = s.shape
    rows = np.full((Q, M), -1, dtype=np.int32)
    sc = np.full((Q, M), -np.inf, dtype=np.float32)
    ar = np.arange(N)
    for i in range(Q):
        order = np.lexsort((ar, -s[i]))
        order = order[np.isfinite(s[i, order])][:M]
        rows[i, :len(order)] = order
        sc[i, :len(order)] = s[i, order].astype(np.float32)
    return sc, rows


def shortlist_ref(q_bf, items_bf, M, excl=None):
    return first_m(mask_rows(approx_scores(q_bf, items_bf), excl), M)


def rescore_ref(s_exact, rows, k):
    """The re-scored list of int rows [Q, M] on fp64 scores [Q, N]: entries outside [0, N) are no
    candidates, a row named twice appears twice; (scores f32 [Q, k], rows int32 [Q, k])."""
    Q, N = s_exact.shape
    out_r = np.full((Q, k), -1, dtype=np.int32)
    out_s = np.full((Q, k), -np.inf, dtype=np.float32)
    for i in range(Q):
        r = np.asarray(rows[i])
        r = r[(r >= 0) & (r < N)]
        order = np.lexsort((r, -s_exact[i, r]))[:k]
        out_r[i, :len(order)] = r[order]
        out_s[i, :len(order)] = s_exact[i, r[order]].astype(np.float32)
    return out_s, out_r


def two_stage_ref(q_bf, items_bf, M, k, excl=None):
    """The flat list restricted to the restatement's shortlist."""
    _, rows = shortlist_ref(q_bf, items_bf, M, excl)
    return rescore_ref(exact_scores(q_bf, items_bf), rows, k)


def holds_with_margin(q_bf, items_bf, want_rows, M, excl=None, margin=EPS):
    """bool [Q]: every row of want_rows [Q, k] (entries < 0 skipped) scores more than `margin` above the
    M-th approximate score of its query (or fewer than M rows are eligible), so a shortlist that obeys
    the eps rules must hold it.  A condition on the inputs alone."""
    s = mask_rows(approx_scores(q_bf, items_bf), excl)
    out = np.zeros(s.shape[0], dtype=bool)
    for i in range(s.shape[0]):
        fin = np.sort(s[i][np.isfinite(s[i])])[::-1]
        cut = fin[M - 1] if len(fin) >= M else -np.inf
        r = np.asarray(want_rows[i])
        r = r[r >= 0]
        out[i] = bool((s[i, r] > cut + margin).all())
    return out


def unit_case(Q, N, clustered, seed):
    """(q f32 [Q, 128] bf16-representable unit rows that normalise to themselves, items bf16 [N, 128]);
    clustered: 16 centres, noise 0.3."""
    key = ("unit", Q, N, clustered, seed)
    if key not in _CACHE:
        g = torch.Generator().manual_seed(seed)
        if clustered:
            cen = torch.randn(16, D, generator=g)
            x = cen[torch.randint(0, 16, (N,), generator=g)] + 0.3 * torch.randn(N, D, generator=g)
            y = cen[torch.randint(0, 16, (Q,), generator=g)] + 0.3 * torch.randn(Q, D, generator=g)
        else:
            x = torch.randn(N, D, generator=g)
            y = torch.randn(Q, D, generator=g)
        items = F.normalize(x, dim=-1).to(torch.bfloat16)
        q = F.normalize(y, dim=-1).to(torch.bfloat16).float()
        assert torch.equal(F.normalize(q, dim=-1).to(torch.bfloat16).float(), q)
        _CACHE[key] = (q, items)
    return _CACHE[key]


def int_case(Q, N, seed=77):
    """Integer rows in -3..3 whose amax cycles through 1, 2, 3 (queries too): every code and product
    is exact, so the approximate score is the flat score whatever the accumulation order."""
    key = ("int", Q, N, seed)
    if key not in _CACHE:
        g = torch.Generator().manual_seed(seed)

        def rows(n):
            c = (torch.arange(n) % 3 + 1)[:, None]
            x = (torch.randint(-3, 4, (n, D), generator=g).clamp(-c, c)).float()
            x[torch.arange(n), torch.randint(0, D, (n,), generator=g)] = c[:, 0].float()
            return x
        _CACHE[key] = (rows(Q), rows(N).to(torch.bfloat16))
    return _CACHE[key]


def edge_rows():
    """bf16 [R, 128]: the quantiser's edge rows."""
    r = []
    z = torch.zeros(D)
    r.append(z.clone())                                            # zero row
    for p in (-3, 0, 5):
        x = z.clone(); x[7] = 0.875 * 2.0 ** p; x[9] = -0.3 * 2.0 ** p; r.append(x)   # amax = 0.875 2^p
        x = z.clone(); x[7] = -(0.875 + 2.0 ** -8) * 2.0 ** p; x[9] = 0.3 * 2.0 ** p; r.append(x)  # the next bf16 above
    x = z.clone(); x[100] = -1.3; r.append(x)                      # a single non-zero element
    x = z.clone(); x[0] = 1.0; x[1] = 2.0 ** -18; x[2] = -2.0 ** -19; x[3] = 2.0 ** -30; r.append(x)  # below the subnormals
    x = z.clone(); x[0] = 1.0; x[1] = 2.0 ** -17; x[2] = 3 * 2.0 ** -18; x[3] = 2.0 ** -16; r.append(x)  # ties, subnormals
    x = torch.linspace(-1, 1, D) * 2.0 ** -60; r.append(x)          # amax near 2^-60
    x = torch.linspace(-1, 1, D) * 2.0 ** 60; r.append(x)           # amax near 2^60
    out = torch.stack(r).to(torch.bfloat16)
    assert torch.equal(out[1].float().abs().amax(), torch.tensor(0.875 * 2.0 ** -3))
    return out


def check_eps_rules(s, M, g_scores, g_rows, eps=EPS):
    """The eps rules of tests/test_gpu_retrieval.py on fp64 scores s [Q, N] with -inf for ineligible
    rows: scores within eps, every row above the M-th score + eps present, none below it - eps,
    order consistent, the tail (-inf, -1).  At most 4 rows may lie within eps of the cut-off: a
    condition on s alone, checked before the device's output is looked at."""
    Q, N = s.shape
    cuts = []
    for i in range(Q):
        fin = np.sort(s[i][np.isfinite(s[i])])[::-1]
        kk = min(M, len(fin))
        kth = fin[kk - 1] if kk else np.inf
        cuts.append((kk, kth))
        assert int((np.abs(s[i] - kth) <= eps).sum()) <= 4, "too many catalogue rows within eps of the M-th score"
    for i in range(Q):
        kk, kth = cuts[i]
        r = g_rows[i, :kk]
        assert (r >= 0).all() and (r < N).all() and len(set(r.tolist())) == kk, i
        assert (g_rows[i, kk:] == -1).all() and np.isneginf(g_scores[i, kk:]).all(), i
        assert np.isfinite(s[i, r]).all(), i
        assert np.abs(g_scores[i, :kk].astype(np.float64) - s[i, r]).max() <= eps, i
        must = np.nonzero(s[i] > kth + eps)[0]
        assert set(must.tolist()) <= set(r.tolist()), i
        assert (s[i, r] >= kth - eps).all(), i
        assert (np.diff(g_scores[i, :kk]) <= 0).all(), i
