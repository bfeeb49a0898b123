"""Shared by test_retrieval_ivf_host.py and test_gpu_retrieval_ivf.py: the fp64 checker of the
clustered scan (lthm_retrieve_ivf_topk) and the synthetic catalogues of its tests.

Exact cases hold small integers (exact in bf16; every dot product and every partial sum is an
integer far below 2^24, so every summation order gives the same f32) and are compared bit for bit.
"""
import numpy as np
import torch

D = 128


def ivf_checker(q_bf, emb_bf, row_ids, list_off, probes, k, exclude_rows=None):
    """q_bf [Q, 128], emb_bf [N, 128] (the clustered rows): the bf16 operands; row_ids int64 [N],
    list_off int64 [L + 1], probes int [Q, P], exclude_rows int [Q, X] (clustered rows) or None, all
    CPU tensors.  Returns (s fp64 [Q, N], scores f32 [Q, k], ids int64 [Q, k], allowed): per query the
    rows of the probe row's valid lists (entries outside [0, L) are ignored; a list named twice
    counts twice, as the merge's duplicate rule has it) without the excluded rows, sorted by (score
    descending, id ascending), the first k, then (-inf, 0).  allowed[q] is the sorted array of the
    query's eligible rows."""
    s = (q_bf.double() @ emb_bf.double().T).numpy()
    ids = row_ids.numpy()
    off = list_off.numpy()
    L = len(off) - 1
    Q = s.shape[0]
    out_s = np.full((Q, k), -np.inf, dtype=np.float32)
    out_i = np.zeros((Q, k), dtype=np.int64)
    allowed = []
    for i in range(Q):
        rows = [np.arange(off[c], off[c + 1]) for c in probes[i].tolist() if 0 <= c < L]
        rows = np.concatenate(rows) if rows else np.zeros(0, dtype=np.int64)
        if exclude_rows is not None:
            rows = rows[~np.isin(rows, exclude_rows[i].numpy())]
        order = np.lexsort((ids[rows], -s[i, rows]))[:k]
        out_s[i, :order.size] = (s[i, rows[order]] + 0.0).astype(np.float32)
        out_i[i, :order.size] = ids[rows[order]]
        allowed.append(np.unique(rows))
    return s, out_s, out_i, allowed


def brute_force(q_bf, emb_bf, row_ids, list_off, probes, k):
    """The same list by a plain Python sort over (score, id) tuples: the checker's own check."""
    out = []
    for i in range(q_bf.shape[0]):
        cand = []
        for c in probes[i].tolist():
            if 0 <= c < len(list_off) - 1:
                for r in range(int(list_off[c]), int(list_off[c + 1])):
                    cand.append((-float(q_bf[i].double() @ emb_bf[r].double()), int(row_ids[r])))
        cand.sort()
        out.append(cand[:k])
    return out


def spread_ids(n, seed):
    """n distinct non-zero int64 ids, ascending: negative ones, small ones and ones above 2^32."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.unique(torch.cat([torch.randint(-(1 << 40), -1, (n,), generator=g),
                                  torch.randint(1, 50000, (n,), generator=g),
                                  torch.randint(1 << 33, 1 << 50, (n,), generator=g)]))
    pick = torch.randperm(ids.numel(), generator=g)[:n]
    return torch.sort(ids[pick])[0]


SHAPE_LENGTHS = [63, 0, 130, 1, 64]  # an empty list, a sub-tile list, one tile, two tiles and a tail
BIG = 2                              # the 130-row list, which every query probes
SHAPE_Q = 70


def shapes_case():
    """L = 5 lists of SHAPE_LENGTHS rows, N = 258, Q = 70.  The lists' ids interleave (a seeded
    permutation of the labels over the ascending ids), so the merge's id tie-break across lists
    decides.  Items: 24 distinct rows in {-2..2} repeated at random, so every score comes in a tie
    run; coordinate 0 of every item is 0.  Queries in {-2..2} with q[:, 0] = 2; centroid BIG is
    256 e_0 (score 512 for every query, above any other centroid's |score| <= 2 * 127), the other
    centroids hold {-1, 0, 1} with coordinate 0 zero: every query's first probe is BIG, its others
    vary.  Returns a dict of CPU tensors: ids, emb (flat, id-ascending), assign, centroids, tags
    (1 << list), q."""
    g = torch.Generator().manual_seed(4242)
    L, N = len(SHAPE_LENGTHS), sum(SHAPE_LENGTHS)
    labels = torch.cat([torch.full((n,), c, dtype=torch.int64) for c, n in enumerate(SHAPE_LENGTHS)])
    assign = labels[torch.randperm(N, generator=g)]
    ids = spread_ids(N, 11)
    base = torch.randint(-2, 3, (24, D), generator=g)
    base[:, 0] = 0
    emb = base[torch.randint(0, 24, (N,), generator=g)].to(torch.bfloat16)
    q = torch.randint(-2, 3, (SHAPE_Q, D), generator=g).float()
    q[:, 0] = 2.0
    cen = torch.randint(-1, 2, (L, D), generator=g).float()
    cen[:, 0] = 0.0
    cen[BIG] = 0.0
    cen[BIG, 0] = 256.0
    return dict(ids=ids, emb=emb, assign=assign, centroids=cen.to(torch.bfloat16), tags=(1 << assign).to(torch.int32), q=q)


def shapes_exclude(case, X):
    """exclude_ids int64 [Q, X] for the shapes case: ids from all over the catalogue (so also of
    lists a query does not probe), the pad id 0 and ids the catalogue does not hold.  With X = 1,024
    query 0 lists every id of the BIG list (a whole probed list) and query 1 every id of the
    catalogue; with X = 1 query 1 names an unknown id and query 2 the pad."""
    g = torch.Generator().manual_seed(900 + X)
    ids, N = case["ids"], case["ids"].numel()
    ex = ids[torch.randint(0, N, (SHAPE_Q, X), generator=g)].clone()
    if X == 1:
        ex[1, 0] = 987654321098
        ex[2, 0] = 0
        return ex
    ex[:, ::9] = 0
    ex[:, 1::9] = 987654321098
    big = ids[case["assign"] == BIG]
    ex[0, :big.numel()] = big
    ex[1, :N] = ids
    return ex


PRUNE_LENGTHS = [5, 4096, 64, 70]


def prune_case():
    """One list of 4,096 rows whose score ascends with the row for every query, and three short
    lists.  Row i of the long list holds i spread over coordinates 0..15 (values <= 256, exact in
    bf16) and zeros elsewhere; the queries are v (ones on 0..15), 2 v and v plus {-1, 0, 1} on the
    coordinates the long list does not use, so the long list scores i, 2 i and i: every row passes
    the threshold and the prune runs at every tile.  The short lists hold {-2..2} everywhere."""
    g = torch.Generator().manual_seed(77)
    L, N = len(PRUNE_LENGTHS), sum(PRUNE_LENGTHS)
    labels = torch.cat([torch.full((n,), c, dtype=torch.int64) for c, n in enumerate(PRUNE_LENGTHS)])
    assign = labels[torch.randperm(N, generator=g)]
    ids = spread_ids(N, 12)
    emb = torch.randint(-2, 3, (N, D), generator=g).float()
    i = torch.arange(4096)
    long_rows = torch.zeros((4096, D))
    long_rows[:, :16] = (i // 16)[:, None] + (torch.arange(16)[None, :] < (i % 16)[:, None]).float()
    emb[assign == 1] = long_rows  # in id order: ascending with the row of the list
    v = torch.zeros(D)
    v[:16] = 1.0
    w = torch.randint(-1, 2, (D,), generator=g).float()
    w[:16] = 0.0
    q = torch.stack([v, 2 * v, v + w])
    cen = torch.randint(-1, 2, (L, D), generator=g).to(torch.bfloat16)
    return dict(ids=ids, emb=emb.to(torch.bfloat16), assign=assign, centroids=cen, tags=(1 << assign).to(torch.int32), q=q)


def unit_case(N, L, Q, seed):
    """N unit vectors around L random unit centres (the centres are the centroids, every item is
    assigned to the centre it was drawn around), Q unit queries near some of the centres.  The
    queries' f32 values are bf16-representable, so normalising them again gives back the same bf16."""
    g = torch.Generator().manual_seed(seed)
    cen = torch.nn.functional.normalize(torch.randn(L, D, generator=g), dim=1)
    assign = torch.randint(0, L, (N,), generator=g)
    emb = torch.nn.functional.normalize(cen[assign] + 0.5 * torch.randn(N, D, generator=g) / D ** 0.5, dim=1)
    q = torch.nn.functional.normalize(cen[torch.randint(0, L, (Q,), generator=g)]
                                      + 0.5 * torch.randn(Q, D, generator=g) / D ** 0.5, dim=1)
    q = q.to(torch.bfloat16).float()
    ids = torch.arange(1, N + 1, dtype=torch.int64) * 7 - 3
    return dict(ids=ids, emb=emb.to(torch.bfloat16), assign=assign, centroids=cen.to(torch.bfloat16), q=q)
