"""Shared by test_retrieval_ivf_deep_host.py and test_gpu_retrieval_ivf_deep.py: the exact catalogue of
the deep clustered scan's tests (lthm_retrieve_ivf_topk_deep, k up to 1,024) and its exclusion lists.

The fp64 checker is retrieval_ivf_filt_case.ivf_filt_checker, which takes any k; the host test checks it
against a brute-force sort at k > 128.  Data is exact, as in retrieval_ivf_filt_case.py: integer-valued
embeddings, biases that are multiples of 1/8 with |bias| <= 32 and weights in {-1, 0, 0.5, 1, 2}.  The
largest |dot| here is 4,095 + 2 * 2 * 112, so fmaf(weight, bias, dot) needs 13 integer and 4 fractional
bits: exact in f32, and nothing is tolerated.
"""
import torch

from retrieval_ivf_case import D, spread_ids
from retrieval_ivf_filt_case import (LIST_SHIFT, exact_bias, ivf_filt_checker, brute_force_filt,  # noqa: F401
                                     restrict_to_probes, shape_cursors, shape_filters, shape_weights, user_tags)

# an empty list, one row, a sub-tile list, one tile, two tiles and a tail, a list longer than k = 1,024, RD_LIM + 1
# rows (the first length at which an append sets the prune flag), RD_CAP, RD_CAP + 1 (the first length at which the
# flag is read) and the long list
DEEP_LENGTHS = [0, 1, 63, 64, 130, 1030, 1985, 2048, 2049, 4096]
LONG = 9   # the 4,096-row list, which every query probes first
DEEP_Q = 70  # more than 64 pairs on the long list: two pair tiles
DEEP_KS = [129, 200, 1024]


def deep_case():
    """L = 10 lists of DEEP_LENGTHS rows, N = 11,466, Q = 70; the lists' ids interleave (a seeded
    permutation of the labels over the ascending ids), so the merge's id tie-break across lists decides.
    Row i of the long list holds i spread over coordinates 0..15 (values <= 256, exact in bf16) and zeros
    elsewhere; every other item holds one of 24 rows in {-2..2} on coordinates 16..127 and zeros on
    0..15, so its scores come in tie runs.  Every query is 1 on coordinates 0..15 and {-2..2} elsewhere:
    it scores row i of the long list as i exactly, ascending with the row, so every tile of that list
    appends for every pair and the prune runs again and again.  The long list's centroid is 64 on
    coordinates 0..15 (score 1,024, above any other centroid's |score| <= 2 * 112), the other centroids
    hold {-1, 0, 1} on 16..127: every query's first probe is LONG, its others vary.  Returns a dict of CPU
    tensors: ids, emb (flat, id-ascending), assign, centroids, q."""
    g = torch.Generator().manual_seed(9090)
    L, N = len(DEEP_LENGTHS), sum(DEEP_LENGTHS)
    labels = torch.cat([torch.full((n,), c, dtype=torch.int64) for c, n in enumerate(DEEP_LENGTHS)])
    assign = labels[torch.randperm(N, generator=g)]
    ids = spread_ids(N, 13)
    base = torch.randint(-2, 3, (24, D), generator=g).float()
    base[:, :16] = 0.0
    emb = base[torch.randint(0, 24, (N,), generator=g)]
    i = torch.arange(4096)
    long_rows = torch.zeros((4096, D))
    long_rows[:, :16] = (i // 16)[:, None] + (torch.arange(16)[None, :] < (i % 16)[:, None]).float()
    emb[assign == LONG] = long_rows  # in id order: ascending with the row of the list
    q = torch.randint(-2, 3, (DEEP_Q, D), generator=g).float()
    q[:, :16] = 1.0
    cen = torch.randint(-1, 2, (L, D), generator=g).float()
    cen[:, :16] = 0.0
    cen[LONG] = 0.0
    cen[LONG, :16] = 64.0
    return dict(ids=ids, emb=emb.to(torch.bfloat16), assign=assign, centroids=cen.to(torch.bfloat16), q=q)


def deep_exclude(case, X):
    """exclude_ids int64 [Q, X]: ids from all over the catalogue (so also of lists a query does not probe),
    the pad id 0 and ids the catalogue does not hold.  With X = 1,024 query 0 lists the 1,024 best rows of
    the long list (its whole k = 1,024 list at nprobe = 1) and query 1 the whole 1,030-row list's first
    1,024 ids; with X = 1 query 1 names an unknown id and query 2 the pad."""
    g = torch.Generator().manual_seed(700 + X)
    ids, N = case["ids"], case["ids"].numel()
    ex = ids[torch.randint(0, N, (DEEP_Q, X), generator=g)].clone()
    if X == 1:
        ex[1, 0] = 987654321098
        ex[2, 0] = 0
        return ex
    ex[:, ::9] = 0
    ex[:, 1::9] = 987654321098
    ex[0] = ids[case["assign"] == LONG][-X:]
    ex[1] = ids[case["assign"] == 5][:X]
    return ex
