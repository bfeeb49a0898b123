"""Shared by test_retrieval_ivf_group_host.py and test_gpu_retrieval_ivf_group.py: the catalogue, the
grouped queries and the fp64 reference of the clustered scan with several queries per user
(lthm_retrieve_ivf_topk_group).

Exact data only, as in retrieval_ivf_case.py: items and queries hold small integers (exact in bf16; every
dot product and every partial sum is an integer far below 2^24, so every summation order gives the same
f32), biases are multiples of 1/8 and weights come from retrieval_ivf_filt_case.WEIGHTS, so the fp64 value
rounded to f32 is the kernel's f32 and every comparison is bit for bit: the bound on a score is zero, as
it is for that case.
"""
import os
import re

import numpy as np
import torch

from retrieval_ivf_case import D, spread_ids
from retrieval_ivf_filt_case import exact_bias, shape_filters, shape_weights  # noqa: F401  (re-exported)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def scan_tile_rows():
    """The item rows of one scan tile, read from the kernel's source (RT_IT)."""
    with open(os.path.join(ROOT, "recommendations_amd", "csrc", "retrieve.hip")) as f:
        return int(re.search(r"constexpr int RT_IT = (\d+);", f.read()).group(1))


def tile_pairs(G):
    """The (user, probe) pairs one block serves: G adjacent columns per pair inside a row of 16."""
    return 4 * (16 // G)


L = 16
EMPTY, SINGLE, LONG = 3, 9, 6  # the lists of 0 rows, of 1 row and of more than two tiles with a tail
U_MAX, G_MAX = 70, 8
USER_A, USER_B = 5, 11         # the centroids the probe-order user's heads 0 and 1 point at
PROBE_USER, SHORT_USER = 2, 3  # that user, and the user whose two nearest lists are EMPTY and SINGLE


def list_lengths():
    it = scan_tile_rows()
    n = [211, 97, 300, 0, 64, 255, 2 * it + 37, 129, 310, 1, 63, 401, 190, 128, 333, 352]
    n[EMPTY], n[SINGLE], n[LONG] = 0, 1, 2 * it + 37
    return n


def group_case():
    """N = 2,999 rows in L = 16 lists of list_lengths() rows; ids spread over int64 and shuffled against
    the row order (the list of an id is a seeded permutation, so ids interleave across lists and the
    merge's id tie-break decides).  Items: 150 distinct rows in {-2..2} repeated at random, so every
    score comes in a tie run inside a list and across lists; on top, item 1 of list 0 is copied to
    item 2 of list 0 and to item 0 of list 1 (planted ties inside one list and across two).  Coordinates
    0..15 of every item are 0: they carry the probe alone.  Centroid c is 16 e_c.

    Queries q [70, 8, 128] in {-2..2} (coordinates 0..15 in {-1, 0, 1}), with, for the one-slot rule:
      u % 4 == 0   head 1 is head 0: every row scores the same for both
      u % 4 == 1   head 0 is the planted item r(u)'s own vector (its best match by Cauchy-Schwarz among rows
                   of its norm) and head 1 is head 0 plus a vector orthogonal to r(u): r(u) scores the same,
                   its maximum, for both
    PROBE_USER: head 0 points at centroid USER_A alone and head 1 at USER_B alone (every other centroid
    scores below both).  SHORT_USER: every head points at EMPTY and SINGLE.
    Returns CPU tensors: ids, emb (flat, id-ascending), assign, centroids, tags, bias, q, planted."""
    g = torch.Generator().manual_seed(2024)
    lens = list_lengths()
    N = sum(lens)
    labels = torch.cat([torch.full((n,), c, dtype=torch.int64) for c, n in enumerate(lens)])
    assign = labels[torch.randperm(N, generator=g)]
    ids = spread_ids(N, 21)
    base = torch.randint(-2, 3, (150, D), generator=g)
    emb = base[torch.randint(0, 150, (N,), generator=g)].clone()
    emb[:, :16] = 0
    in0, in1 = torch.nonzero(assign == 0)[:, 0], torch.nonzero(assign == 1)[:, 0]
    emb[in0[2]] = emb[in0[1]]
    emb[in1[0]] = emb[in0[1]]
    q = torch.randint(-2, 3, (U_MAX, G_MAX, D), generator=g).float()
    q[:, :, :16] = torch.randint(-1, 2, (U_MAX, G_MAX, 16), generator=g).float()
    planted = {}
    for u in range(U_MAX):
        if u % 4 == 0:
            q[u, 1] = q[u, 0]
        elif u % 4 == 1:
            r = int(torch.randint(0, N, (1,), generator=g))
            e = emb[r].float()
            i, j = [int(x) for x in torch.nonzero(e == e[torch.nonzero(e)[0, 0]])[:2, 0]]  # two equal non-zero entries
            q[u, 0, 16:] = e[16:]
            q[u, 1] = q[u, 0]
            q[u, 1, i] += 1.0
            q[u, 1, j] -= 1.0
            planted[u] = int(ids[r])
    q[PROBE_USER, :, :16] = -1.0
    q[PROBE_USER, 0, USER_A] = 1.0
    q[PROBE_USER, 1, USER_B] = 1.0
    q[SHORT_USER, :, :16] = -1.0
    q[SHORT_USER, :, EMPTY] = 1.0
    q[SHORT_USER, :, SINGLE] = 1.0
    cen = torch.zeros((L, D))
    cen[torch.arange(L), torch.arange(L)] = 16.0
    tags = torch.randint(0, 32, (N,), generator=g).to(torch.int32)
    return dict(ids=ids, emb=emb.to(torch.bfloat16), assign=assign, centroids=cen.to(torch.bfloat16), tags=tags,
                bias=exact_bias(N, 22), q=q, planted=planted)


def exclude_ids(case, U, X=40):
    """int64 [U, X]: ids from all over the catalogue, the pad id 0 and ids the catalogue does not hold."""
    g = torch.Generator().manual_seed(700 + X)
    ids = case["ids"]
    ex = ids[torch.randint(0, ids.numel(), (U, X), generator=g)].clone()
    ex[:, ::9] = 0
    ex[:, 1::9] = 987654321098
    return ex


def group_checker(q_bf, emb_bf, row_ids, list_off, probes, k, bias=None):
    """q_bf [U, G, 128] and emb_bf [N, 128] (the clustered rows): the bf16 operands; row_ids int64 [N],
    list_off int64 [L + 1], probes int [U, P]; bias f32 [N] in the clustered order or None (weight 1, added
    behind the maximum); CPU tensors.  Returns (s fp64 [U, N] = max_g of the fp64 dots (+ bias), scores
    f32 [U, k], ids int64 [U, k]): per user the rows of the probed lists by (score descending, id
    ascending), each once, the first k, then (-inf, 0)."""
    s = torch.einsum("ugd,nd->ugn", q_bf.double(), emb_bf.double()).max(dim=1)[0].numpy()
    if bias is not None:
        s = s + bias.double().numpy()[None, :]
    ids, off = row_ids.numpy(), list_off.numpy()
    U = s.shape[0]
    out_s = np.full((U, k), -np.inf, dtype=np.float32)
    out_i = np.zeros((U, k), dtype=np.int64)
    for u in range(U):
        rows = [np.arange(off[c], off[c + 1]) for c in probes[u].tolist() if 0 <= c < len(off) - 1]
        rows = np.concatenate(rows) if rows else np.zeros(0, dtype=np.int64)
        order = np.lexsort((ids[rows], -s[u, rows]))[:k]
        out_s[u, :order.size] = (s[u, rows[order]] + 0.0).astype(np.float32)
        out_i[u, :order.size] = ids[rows[order]]
    return s, out_s, out_i
