"""Shared by test_rank_host.py and test_gpu_rank.py: the checker of the ranking stage's order, the
explicit batch that K.rank_assemble must reproduce bit for bit, and the hand-made lists of the sort tests.

The order (csrc/rank.hip): an entry (logit, row) at list position src is a candidate when row >= 0 and
the logit is not NaN; candidates come by (logit descending, row ascending, src ascending), -0.0 equal to
+0.0 and +-inf ordinary values; the slots behind the last candidate hold (-inf, -1, -1).  The checker
states that with one numpy lexsort per list, in the logits' own f32: nothing is computed, so there is no
rounding to bound and every comparison against it is exact.
"""
import numpy as np
import torch

SORT_M = (1, 2, 63, 64, 65, 1000, 1024)


def sort_ks(M):
    return sorted({1, M // 2 or 1, M})


def sort_checker(logits, rows, k):
    """(scores f32 [Q, k], rows int32 [Q, k], src int32 [Q, k]) of f32 [Q, M] logits and int32 [Q, M] rows."""
    logits = np.asarray(logits, dtype=np.float32)
    rows = np.asarray(rows, dtype=np.int32)
    Q, M = logits.shape
    assert rows.shape == (Q, M) and 1 <= k <= M
    out_s = np.full((Q, k), -np.inf, dtype=np.float32)
    out_r = np.full((Q, k), -1, dtype=np.int32)
    out_src = np.full((Q, k), -1, dtype=np.int32)
    for q in range(Q):
        src = np.nonzero((rows[q] >= 0) & ~np.isnan(logits[q]))[0]
        l, r = logits[q, src], rows[q, src]
        order = np.lexsort((src, r, -l))[:k]  # the last key is the primary one; -(-0.0) == -(+0.0)
        n = order.size
        out_s[q, :n], out_r[q, :n], out_src[q, :n] = l[order], r[order], src[order]
    return out_s, out_r, out_src


def brute_force(logits, rows, k):
    """The same lists by Python's sort on (-logit, row, src) tuples: [(logit, row, src), ...] per list."""
    out = []
    for lq, rq in zip(logits, rows):
        cand = [(-float(l), int(r), m) for m, (l, r) in enumerate(zip(lq, rq)) if int(r) >= 0 and float(l) == float(l)]
        out.append([(-a, r, m) for a, r, m in sorted(cand)[:k]])
    return out


def explicit_batch(user_dense, user_cat, item_dense, item_cat, rows):
    """The batch of K.rank_assemble built with expand / index / cat: (dense f32 [Q M, Du + Di], cat int64
    [Q M, Fu + Fi]); a row index outside [0, N) gives item columns of zeros."""
    Q, M = rows.shape
    N = item_dense.shape[0]
    ok = ((rows >= 0) & (rows < N))[..., None]
    idx = rows.long().clamp(0, max(N - 1, 0))
    i_dense = torch.where(ok, item_dense[idx], torch.zeros((), dtype=item_dense.dtype, device=rows.device))
    i_cat = torch.where(ok, item_cat[idx], torch.zeros((), dtype=item_cat.dtype, device=rows.device))
    dense = torch.cat([user_dense[:, None, :].expand(Q, M, -1), i_dense], dim=-1)
    cat = torch.cat([user_cat[:, None, :].expand(Q, M, -1), i_cat], dim=-1)
    return dense.reshape(Q * M, -1).contiguous(), cat.reshape(Q * M, -1).contiguous()


def assemble_case(M, Du, Di, Fu, Fi, Q=3, N=200, seed=0):
    """Inputs of K.rank_assemble on the CPU: pads of -1 and of N at the first, a middle and the last
    position of lists 0 and 1, and list 2 all pads."""
    g = torch.Generator().manual_seed(seed + 7 * M + Du)
    t = dict(user_dense=torch.randn((Q, Du), generator=g), user_cat=torch.randint(-(2 ** 62), 2 ** 62, (Q, Fu), generator=g),
             item_dense=torch.randn((N, Di), generator=g), item_cat=torch.randint(-(2 ** 62), 2 ** 62, (N, Fi), generator=g))
    rows = torch.randint(0, N, (Q, M), generator=g).to(torch.int32)
    for q, pad in ((0, -1), (1, N)):
        for m in (0, M // 2, M - 1):
            rows[q, m] = pad
    rows[0, M // 2] = N  # both kinds in one list as well
    rows[2] = torch.where(torch.arange(M) % 2 == 0, -1, N + 5).to(torch.int32)
    rows[2, 0] = -(2 ** 31)
    rows[2, M - 1] = 2 ** 31 - 1
    t["rows"] = rows
    return t


def _mixed(M, seed):
    rng = np.random.default_rng(1000 * M + seed)
    special = [(np.nan, 5), (np.inf, 7), (-np.inf, 9), (-0.0, 11), (0.0, 10), (1.5, 42), (1.5, 42), (2.0, -1),
               (np.inf, 3), (-np.inf, 2), (0.0, 11), (np.nan, -1)]
    special = special[seed % len(special):] + special[:seed % len(special)]
    nb = min(100, max(0, M - len(special)) // 2)  # the block of equal logits, its rows shuffled
    block = [(0.25, int(r)) for r in rng.permutation(np.arange(1000, 1000 + nb))]
    rest = []
    for _ in range(max(0, M - len(special) - nb)):
        row = int(rng.integers(0, 500))
        if rng.random() < 0.1:
            row = -1 if rng.random() < 0.5 else -7
        rest.append((float(np.round(rng.normal() * 4) / 4 + 0.0), row))  # quarters: many ties across rows; no -0.0
    ent = (special + block + rest)[:M]
    if M > len(special):  # scatter everything; -0.0 and the +0.0 behind it move as one unit
        units, i = [], 0
        while i < len(ent):
            pair = i + 1 < len(ent) and ent[i][1] == 11 and np.signbit(ent[i][0]) and ent[i + 1] == (0.0, 10)
            units.append(ent[i:i + 2] if pair else ent[i:i + 1])
            i += 2 if pair else 1
        ent = [e for u in rng.permutation(len(units)) for e in units[u]]
    return ent


def sort_case(M):
    """(logits f32 [7, M], rows int32 [7, M]): three mixed lists (NaN, +inf, -inf, -0.0 next to +0.0, a block
    of up to 100 equal logits with shuffled rows, one row twice with equal logits, pads scattered through;
    a list shorter than that holds what fits), a list of pads, a list of NaN, a sorted list and its
    reverse."""
    logits = np.zeros((7, M), dtype=np.float32)
    rows = np.zeros((7, M), dtype=np.int32)
    for q in range(3):
        ent = _mixed(M, q)
        logits[q] = [e[0] for e in ent]
        rows[q] = [e[1] for e in ent]
    logits[3] = np.arange(M, dtype=np.float32)
    rows[3] = np.where(np.arange(M) % 3 == 0, -1, -5)
    logits[4] = np.nan
    rows[4] = np.arange(M)
    logits[5] = (M - np.arange(M)).astype(np.float32) / 2
    rows[5] = np.arange(M)
    logits[6], rows[6] = logits[5, ::-1], rows[5, ::-1]
    return logits, rows
