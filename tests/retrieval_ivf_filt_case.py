"""Shared by test_retrieval_ivf_filt_host.py and test_gpu_retrieval_ivf_filt.py: the fp64 checker of the
clustered scan with tag filters, a score prior and a cursor (lthm_retrieve_ivf_topk_filt), its own
check by a brute-force sort, and the tags / bias / weights / filters of the exact cases.

Exact data only: the items and queries of retrieval_ivf_case.py (small integers, every dot an integer
far below 2^24), biases that are multiples of 1/8 with |bias| <= 32 and weights in {-1, 0, 0.5, 1, 2}.
Then weight * bias is a multiple of 1/16 of magnitude <= 64 and fmaf(weight, bias, dot) is exact in f32:
the fp64 value below, rounded to f32, is the kernel's f32 bit for bit, and nothing is tolerated.

The tag word of an item is  user bits (low 16) | 1 << (16 + list): the flat catalogue can be restricted
to the probed lists through `none` (the high bits of the lists a query does not probe) while `all`,
`any` and `none` on the low bits are the filter under test.
"""
import numpy as np
import torch

from retrieval_ivf_case import BIG, SHAPE_Q, prune_case, shapes_case, spread_ids  # noqa: F401  (re-exported)

WEIGHTS = [-1.0, 0.0, 0.5, 1.0, 2.0]
LIST_SHIFT = 16
BIG_BIT = 1 << 4  # the user bit that every item of the BIG list carries, and no other item


def tags_pass(tags, filt):
    """bool [N]: retr_topk_k's rule for one filter (all, any, none) over int64 tag words."""
    fall, fany, fnone = (int(x) & 0xFFFFFFFF for x in filt)
    t = tags.astype(np.int64) & 0xFFFFFFFF
    return ((t & fall) == fall) & ((fany == 0) | ((t & fany) != 0)) & ((t & fnone) == 0)


def ivf_filt_checker(q_bf, emb_bf, row_ids, list_off, probes, k, exclude_rows=None, tags=None, tag_filter=None,
                     bias=None, weight=None, after_scores=None, after_ids=None):
    """ivf_checker with the three features.  q_bf [Q, 128] / emb_bf [N, 128]: the bf16 operands (clustered
    rows); tags int32 [N] and bias f32 [N] in the clustered order; tag_filter int [Q, 3]; weight f32 [Q] or
    None (1); after_scores f32 [Q] and after_ids int64 [Q]; all CPU tensors or None.  Returns (s fp64
    [Q, N] with the prior, scores f32 [Q, k], ids int64 [Q, k]): per query the rows of the probed lists
    that are not excluded, pass the filter and lie strictly behind the cursor (s < cs or (s == cs and id >
    after_id), compared in f32, so a NaN or -inf cs admits nothing), by (score descending, id ascending),
    the first k, then (-inf, 0)."""
    s = (q_bf.double() @ emb_bf.double().T).numpy()
    Q, N = s.shape
    if bias is not None:
        w = np.ones(Q) if weight is None else weight.double().numpy()
        s = s + w[:, None] * bias.double().numpy()[None, :]
    ids = row_ids.numpy()
    off = list_off.numpy()
    L = len(off) - 1
    tg = None if tags is None else tags.numpy()
    out_s = np.full((Q, k), -np.inf, dtype=np.float32)
    out_i = np.zeros((Q, k), dtype=np.int64)
    for i in range(Q):
        rows = [np.arange(off[c], off[c + 1]) for c in probes[i].tolist() if 0 <= c < L]
        rows = np.concatenate(rows) if rows else np.zeros(0, dtype=np.int64)
        if exclude_rows is not None:
            rows = rows[~np.isin(rows, exclude_rows[i].numpy())]
        if tag_filter is not None:
            rows = rows[tags_pass(tg[rows], tag_filter[i].tolist())]
        if after_scores is not None:
            cs, aid = np.float32(after_scores[i].item()), int(after_ids[i])
            s32 = s[i, rows].astype(np.float32)
            with np.errstate(invalid="ignore"):
                rows = rows[(s32 < cs) | ((s32 == cs) & (ids[rows] > aid))]
        order = np.lexsort((ids[rows], -s[i, rows]))[:k]
        out_s[i, :order.size] = (s[i, rows[order]] + 0.0).astype(np.float32)
        out_i[i, :order.size] = ids[rows[order]]
    return s, out_s, out_i


def brute_force_filt(q_bf, emb_bf, row_ids, list_off, probes, k, exclude_rows=None, tags=None, tag_filter=None,
                     bias=None, weight=None, after_scores=None, after_ids=None):
    """The same list by a plain Python sort over (-score, id) tuples, one item at a time."""
    out = []
    for i in range(q_bf.shape[0]):
        cand = []
        w = 1.0 if weight is None else float(weight[i])
        for c in probes[i].tolist():
            if not 0 <= c < len(list_off) - 1:
                continue
            for r in range(int(list_off[c]), int(list_off[c + 1])):
                if exclude_rows is not None and r in exclude_rows[i].tolist():
                    continue
                if tag_filter is not None:
                    t = int(tags[r]) & 0xFFFFFFFF
                    fall, fany, fnone = (int(x) & 0xFFFFFFFF for x in tag_filter[i].tolist())
                    if (t & fall) != fall or (fany and not t & fany) or t & fnone:
                        continue
                sc = float(q_bf[i].double() @ emb_bf[r].double())
                if bias is not None:
                    sc += w * float(bias[r])
                if after_scores is not None:
                    cs = float(after_scores[i])
                    if not (sc < cs or (sc == cs and int(row_ids[r]) > int(after_ids[i]))):  # NaN: neither
                        continue
                cand.append((-sc, int(row_ids[r])))
        cand.sort()
        out.append(cand[:k])
    return out


def user_tags(assign, seed):
    """int32 [N] in the order of `assign`: four random user bits, BIG_BIT on the items of the BIG list
    and on no other, and 1 << (16 + list)."""
    g = torch.Generator().manual_seed(seed)
    low = torch.randint(0, 16, assign.shape, generator=g)
    low = low | torch.where(assign == BIG, BIG_BIT, 0)
    return (low | (1 << (LIST_SHIFT + assign))).to(torch.int32)


def exact_bias(n, seed, levels=9):
    """f32 [n]: multiples of 1/8 in [-32, 32], few distinct values so that tie runs survive the prior."""
    g = torch.Generator().manual_seed(seed)
    vals = torch.tensor([-32.0, -4.0, -0.5, -0.125, 0.0, 0.125, 0.375, 2.0, 32.0])[:levels]
    return vals[torch.randint(0, vals.numel(), (n,), generator=g)].contiguous()


def shape_weights(Q):
    """f32 [Q]: the five weights in turn, so 0 and a negative one occur."""
    return torch.tensor([WEIGHTS[i % len(WEIGHTS)] for i in range(Q)], dtype=torch.float32)


def shape_filters(Q, seed):
    """int32 [Q, 3] on the user bits, by query index mod 8:
      0  (0, 0, 0), everything passes          1  unsatisfiable (all & none != 0)
      2  none = BIG_BIT, which empties the BIG list every query probes
      3  all = 0b1111: about one item in 16, fewer than k = 128 whatever is probed
      4  any of two bits                        5  all of one bit, none of another
      6  any = BIG_BIT: the BIG list only       7  random all / any / none over the four bits"""
    g = torch.Generator().manual_seed(seed)
    f = torch.zeros((Q, 3), dtype=torch.int64)
    for i in range(Q):
        m = i % 8
        if m == 1:
            f[i] = torch.tensor([1, 0, 1])
        elif m == 2:
            f[i] = torch.tensor([0, 0, BIG_BIT])
        elif m == 3:
            f[i] = torch.tensor([15, 0, 0])
        elif m == 4:
            f[i] = torch.tensor([0, 6, 0])
        elif m == 5:
            f[i] = torch.tensor([1, 0, 8])
        elif m == 6:
            f[i] = torch.tensor([0, BIG_BIT, 0])
        elif m == 7:
            a, y, n = torch.randint(0, 16, (3,), generator=g).tolist()
            f[i] = torch.tensor([a & ~n & 15, y, n])
    return f.to(torch.int32)


def restrict_to_probes(tag_filter, probes, L):
    """The flat catalogue's filter for the same result: `none` gains the high bit of every list the
    query does not probe.  tag_filter int32 [Q, 3] or None ((0, 0, 0)); probes int [Q, P]."""
    Q = probes.shape[0]
    f = torch.zeros((Q, 3), dtype=torch.int64) if tag_filter is None else tag_filter.cpu().long().clone()
    for i in range(Q):
        probed = {c for c in probes[i].tolist() if 0 <= c < L}
        for c in range(L):
            if c not in probed:
                f[i, 2] |= 1 << (LIST_SHIFT + c)
    return f.to(torch.int32)


def shape_cursors(s, ids, Q, seed):
    """(after_scores f32 [Q], after_ids int64 [Q]) for scores s fp64 [Q, N] over items with ids [N] (any
    order), by query index mod 8: the (score, id) of a seeded item with
      0, 7  the item's own id (inside a tie run, so the id term decides)
      1     id + 1, which the catalogue does not hold     2  the least int64     3  the greatest int64
      4     score +inf                                    5  (-inf, 0), an exhausted page's tail
      6     score NaN"""
    g = torch.Generator().manual_seed(seed)
    held = set(ids.tolist())
    cs = torch.zeros(Q, dtype=torch.float32)
    ci = torch.zeros(Q, dtype=torch.int64)
    for i in range(Q):
        j = int(torch.randint(0, ids.numel(), (1,), generator=g))
        cs[i], ci[i] = float(np.float32(s[i, j])), ids[j]
        m = i % 8
        if m == 1:
            ci[i] = ids[j] + 1
            assert int(ci[i]) not in held
        elif m == 2:
            ci[i] = -(1 << 63)
        elif m == 3:
            ci[i] = (1 << 63) - 1
        elif m == 4:
            cs[i] = float("inf")
        elif m == 5:
            cs[i], ci[i] = float("-inf"), 0
        elif m == 6:
            cs[i] = float("nan")
    return cs, ci


def prune_filt(case):
    """For prune_case(): tags whose bit 0 is set on every other row of the long list (and on every row of
    the short ones), and two priors that ascend with the long list's rows, both used with weight -1.
    `bias_in` keeps the bound of the exact data (multiples of 1/8 in [-32, 32): (i // 8) / 8 - 32): the
    prior alone orders the rows in reverse, but a dot that grows by >= 1 per row outweighs it, so the
    biased score still ascends and the prune runs at every tile under the masks, which is what the case is
    for.  `bias_rev` = 2 i (integers, exact as well, though outside that bound) truly reverses the order
    for the queries that score i: the first tiles fill the list and the threshold rejects the rest."""
    assign = case["assign"]
    N = assign.numel()
    idx = torch.zeros(N, dtype=torch.int64)
    idx[assign == 1] = torch.arange(4096)  # ids ascend, so this is the row inside the list
    low = torch.where(assign == 1, idx % 2, 1)
    tags = (low | (1 << (LIST_SHIFT + assign))).to(torch.int32)
    long = assign == 1
    bias_in = torch.where(long, (idx // 8).float() / 8 - 32, torch.zeros(N))
    bias_rev = torch.where(long, 2.0 * idx.float(), torch.zeros(N))
    return tags, bias_in.contiguous(), bias_rev.contiguous()
