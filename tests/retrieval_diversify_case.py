"""Shared cases and checkers of the diversified-list tests (lthm_retrieve_diversify).

The contract, per query: S empty, d_i = 0; k times, among the candidates not yet selected whose
group key is 0 or shared by fewer than cap selected items, select the first under (m descending,
row ascending, pool position ascending), m_i = lam s_i - (1 - lam) d_i; then d_i = max(d_i, g_ij),
g_ij the dot of rows i and j.  An entry with a row outside [0, N) or a score of -inf / NaN is no
candidate.  Empty slots are (-1, -inf, -inf).

greedy() restates that in fp64.  In the exact cases (rows in {-2..2}, integer scores, lam in {0,
0.5, 1}) every product and sum is an integer or a half below 2^24, so fp64 and every f32 evaluation
order agree and the kernel must match bit for bit.  follow() checks a unit-vector result along the
kernel's own path instead, where a near-tie may legitimately fall either way.
"""
import numpy as np
import torch

D = 128
EPS = 2e-5  # both compared objectives carry lam 7.7e-6 + (1 - lam) 7.7e-6 plus two roundings of values below 2


def _np(t, dtype=None):
    if t is None:
        return None
    a = t.detach().cpu()
    if a.dtype == torch.bfloat16:
        a = a.float()
    a = a.numpy()
    return a if dtype is None else a.astype(dtype)


def _live(rows, scores, N):
    return (rows >= 0) & (rows < N) & ~np.isnan(scores) & ~np.isneginf(scores)


def greedy(rows, scores, items, k, lam=None, groups=None, cap=1):
    """The fp64 greedy: (rows int32 [Q, k], scores f32 [Q, k], objective f32 [Q, k]) as numpy arrays."""
    rows, scores, items, groups = _np(rows, np.int64), _np(scores), _np(items, np.float64), _np(groups, np.int64)
    Q, M = rows.shape
    N = items.shape[0]
    lam = np.ones(Q) if lam is None else _np(lam, np.float64)
    out_r = np.full((Q, k), -1, dtype=np.int32)
    out_s = np.full((Q, k), -np.inf, dtype=np.float32)
    out_o = np.full((Q, k), -np.inf, dtype=np.float32)
    for q in range(Q):
        avail = _live(rows[q], scores[q], N)
        rw = np.where(avail, rows[q], 0)
        X = items[rw]
        s = np.where(avail, scores[q], 0).astype(np.float64)
        key = groups[rw] if groups is not None else np.zeros(M, dtype=np.int64)
        key = np.where(avail, key, 0)
        d = np.zeros(M)
        cnt = np.zeros(M, dtype=np.int64)
        for t in range(k):
            el = avail & ((key == 0) | (cnt < cap))
            if not el.any():
                break
            m = lam[q] * s - (1.0 - lam[q]) * d
            idx = np.flatnonzero(el)
            j = idx[np.lexsort((idx, rw[idx], -m[idx]))[0]]  # m descending, row ascending, position ascending
            out_r[q, t], out_s[q, t], out_o[q, t] = rw[j], scores[q, j], m[j]
            avail[j] = False
            d = np.maximum(d, X @ X[j])
            if key[j] != 0:
                cnt += key == key[j]
    return out_r, out_s, out_o


def brute_force(rows, scores, items, k, lam, groups, cap):
    """The same contract in plain Python over lists: one query, no numpy in the selection."""
    N = len(items)
    cands = [(p, r, s) for p, (r, s) in enumerate(zip(rows, scores)) if 0 <= r < N and s == s and s != float("-inf")]
    chosen, out = [], []
    for _ in range(k):
        best = None
        for p, r, s in cands:
            if any(p == c[0] for c in chosen):
                continue
            if groups is not None and groups[r] != 0 and sum(groups[c[1]] == groups[r] for c in chosen) >= cap:
                continue
            dmax = 0.0
            for c in chosen:
                dmax = max(dmax, sum(a * b for a, b in zip(items[r], items[c[1]])))
            m = lam * s - (1.0 - lam) * dmax
            if best is None or (-m, r, p) < (-best[3], best[1], best[0]):
                best = (p, r, s, m)
        if best is None:
            break
        chosen.append(best)
        out.append((best[1], best[2], best[3]))
    return out


def follow(rows, scores, items, out_rows, out_scores, out_obj, lam=None, groups=None, cap=1, eps=EPS):
    """Check a result along its own path: at every step, from the selected prefix, the chosen candidate
    is eligible and new, its fp64 objective is within eps of the best eligible one, out_obj is within
    eps of it, out_scores holds the pool's own bits, and an empty slot appears only when nothing is
    eligible (and is followed by empty slots only).  Rows of a pool are distinct."""
    rows, scores, items, groups = _np(rows, np.int64), _np(scores), _np(items, np.float64), _np(groups, np.int64)
    out_rows, out_scores, out_obj = _np(out_rows, np.int64), _np(out_scores), _np(out_obj)
    Q, M = rows.shape
    N, k = items.shape[0], out_rows.shape[1]
    lam = np.ones(Q) if lam is None else _np(lam, np.float64)
    for q in range(Q):
        avail = _live(rows[q], scores[q], N)
        rw = np.where(avail, rows[q], 0)
        X = items[rw]
        s = np.where(avail, scores[q], 0).astype(np.float64)
        key = np.where(avail, groups[rw], 0) if groups is not None else np.zeros(M, dtype=np.int64)
        d = np.zeros(M)
        cnt = np.zeros(M, dtype=np.int64)
        for t in range(k):
            el = avail & ((key == 0) | (cnt < cap))
            r = out_rows[q, t]
            if r == -1:
                assert not el.any(), (q, t, "an empty slot while a candidate is eligible")
                assert (out_rows[q, t:] == -1).all() and np.isneginf(out_scores[q, t:]).all() \
                    and np.isneginf(out_obj[q, t:]).all(), (q, t)
                break
            at = np.flatnonzero(avail & (rw == r))
            assert at.size == 1, (q, t, r, "not a candidate, or selected before")
            j = at[0]
            assert el[j], (q, t, r, "over its group's cap")
            m = lam[q] * s - (1.0 - lam[q]) * d
            assert m[j] >= m[el].max() - eps, (q, t, r, float(m[j]), float(m[el].max()))
            assert abs(float(out_obj[q, t]) - m[j]) <= eps, (q, t, float(out_obj[q, t]), float(m[j]))
            assert out_scores[q, t].view(np.int32) == scores[q, j].view(np.int32), (q, t)
            avail[j] = False
            d = np.maximum(d, X @ X[j])
            if key[j] != 0:
                cnt += key == key[j]


EXACT_N = 1100
EXACT_Q = 5
EXACT_LAM = [1.0, 0.5, 0.0, 0.5, 1.0]


def exact_items():
    """N = 1,100 rows: 24 distinct vectors in {-2..2} repeated at random, so dots tie in runs; and one
    group key per row in 0..6 (0 = no group)."""
    g = torch.Generator().manual_seed(2024)
    base = torch.randint(-2, 3, (24, D), generator=g)
    emb = base[torch.randint(0, 24, (EXACT_N,), generator=g)].to(torch.bfloat16)
    groups = torch.randint(0, 7, (EXACT_N,), generator=g).to(torch.int32)
    return emb, groups


def exact_pool(M, seed=0):
    """rows int32 [5, M] (distinct per query, shuffled) and integer scores in -3..3 (tie runs), with
    pools of different live length: query 0 whole; query 1 with padding rows -1 and N in its second
    half; query 2 with -inf and NaN scores on every third entry; query 3 with no candidate at all;
    query 4 whole.  lam per query: EXACT_LAM."""
    g = torch.Generator().manual_seed(1000 + 7 * M + seed)
    rows = torch.stack([torch.randperm(EXACT_N, generator=g)[:M] for _ in range(EXACT_Q)]).to(torch.int32)
    scores = torch.randint(-3, 4, (EXACT_Q, M), generator=g).float()
    half = M // 2
    rows[1, half::2] = -1
    rows[1, half + 1::2] = EXACT_N
    scores[2, 0::3] = float("-inf")
    scores[2, 1::3] = float("nan")
    rows[3, 0::2] = -7
    scores[3, 1::2] = float("-inf")
    return rows, scores, torch.tensor(EXACT_LAM, dtype=torch.float32)
