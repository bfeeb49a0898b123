"""Shared by test_retrieval_shard_host.py and test_gpu_retrieval_shard.py: the numpy model of
lthm_retrieve_merge_shards and the synthetic catalogues of the sharded-retrieval tests."""
import numpy as np
import torch

D = 128
N = 3000
Q = 70


def merge_model(scores, ids, ranks=None):
    """scores f32 [S, Q, k], ids int64 [S, Q, k], ranks int32 [S, Q] or None -> (scores [Q, k], ids
    [Q, k], rank int64 [Q] or None): per query the entries with a score above -inf, sorted by (score
    descending, id ascending) with -0 equal to +0 (returned as +0), the first k of them, then
    (-inf, 0).  rank: -1 if any shard's is -1, else the int64 sum."""
    S, nq, k = scores.shape
    out_s = np.full((nq, k), -np.inf, dtype=np.float32)
    out_i = np.zeros((nq, k), dtype=np.int64)
    for q in range(nq):
        s = scores[:, q].reshape(-1) + np.float32(0.0)  # -0 -> +0
        i = ids[:, q].reshape(-1)
        keep = s > -np.inf
        s, i = s[keep], i[keep]
        order = np.lexsort((i, -s.astype(np.float64)))[:k]
        out_s[q, :order.size] = s[order]
        out_i[q, :order.size] = i[order]
    rank = None
    if ranks is not None:
        r = ranks.astype(np.int64)
        rank = np.where((r == -1).any(axis=0), -1, r.sum(axis=0))
    return out_s, out_i, rank


def merge_case(S, k, nq=5, seed=0):
    """Lists for the merge kernel alone.  Query 0: every list empty; 1: one entry per list; 2: every
    list full; the others: a random fill per list (empty, one entry and full among them).  Scores
    are small integers with -0.0 beside +0.0, so ties run inside and across the lists and the id
    decides at every position; ids are distinct, some negative and some above 2^32."""
    rng = np.random.default_rng(1000 * S + k + seed)
    scores = np.full((S, nq, k), -np.inf, dtype=np.float32)
    ids = np.zeros((S, nq, k), dtype=np.int64)
    vals = np.array([-2.0, -1.0, -0.0, 0.0, 1.0, 2.0], dtype=np.float32)
    for q in range(nq):
        pool = rng.permutation(S * k).astype(np.int64) + 1
        pool = np.where(pool % 3 == 0, -pool, np.where(pool % 3 == 1, pool + (1 << 32) + 5, pool))
        for s in range(S):
            if q == 0:
                n = 0
            elif q == 1:
                n = 1
            elif q == 2:
                n = k
            else:
                n = int(rng.choice([0, 1, k, rng.integers(0, k + 1)]))
            sc = vals[rng.integers(0, len(vals), n)]
            idv = pool[s * k:s * k + n]
            order = np.lexsort((idv, -(sc + np.float32(0.0)).astype(np.float64)))
            scores[s, q, :n] = sc[order]
            ids[s, q, :n] = idv[order]
    ranks = rng.integers(0, 1 << 30, (S, nq)).astype(np.int32)
    ranks[rng.integers(0, S), 1] = -1
    if nq > 3:
        ranks[:, 3] = -1
    return scores, ids, ranks


def catalogue_ids(n=N, seed=5):
    """n distinct non-zero int64 ids, ascending: negative ones, small ones and ones above 2^32."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.unique(torch.cat([torch.randint(-(1 << 40), -1, (n,), generator=g),
                                  torch.randint(1, 50000, (n,), generator=g),
                                  torch.randint(1 << 33, 1 << 50, (n,), generator=g)]))
    pick = torch.randperm(ids.numel(), generator=g)[:n]
    return torch.sort(ids[pick])[0]


def case(kind):
    """kind = "int": operands in {-1, 0, 1}, 48 distinct item rows repeated at random positions (every
    score comes in a tie run spread over the whole catalogue, so across every shard boundary), biases
    in multiples of 0.5 and small integer weights: every f32 is exact.  kind = "unit": unit vectors.
    Returns a dict of CPU tensors: ids, emb, tags, bias, q [Q, 128], q3 [Q, 3, 128], target_ids
    (some held by no shard), exclude_ids (entries from all over the catalogue, pads and unknown
    ids), filt, bw."""
    g = torch.Generator().manual_seed(9091 if kind == "int" else 77)
    ids = catalogue_ids()
    if kind == "int":
        base = torch.randint(-1, 2, (48, D), generator=g)
        emb = base[torch.randint(0, 48, (N,), generator=g)].to(torch.bfloat16)
        q = torch.randint(-1, 2, (Q, D), generator=g).float()
        q3 = torch.randint(-1, 2, (Q, 3, D), generator=g).float()
    else:
        emb = torch.nn.functional.normalize(torch.randn(N, D, generator=g), dim=1).to(torch.bfloat16)
        q = torch.randn(Q, D, generator=g)
        q3 = torch.randn(Q, 3, D, generator=g)
    tags = torch.randint(0, 8, (N,), generator=g).to(torch.int32)
    bias = torch.randint(-4, 5, (N,), generator=g).float() * 0.5
    bw = torch.randint(-1, 3, (Q,), generator=g).float()
    filt = torch.tensor([[1, 0, 0], [0, 6, 0], [0, 0, 4], [0, 0, 0], [1, 2, 4]], dtype=torch.int32).repeat(Q // 5, 1)
    target_ids = ids[(torch.arange(Q) * 7919 + 3) % N].clone()
    target_ids[::5] = 123456789012  # no shard holds it
    target_ids[1] = 0
    excl = ids[torch.randint(0, N, (Q, 37), generator=g)].clone()
    excl[:, ::9] = 0            # pads
    excl[:, 1::9] = 987654321098  # unknown ids
    return dict(ids=ids, emb=emb, tags=tags, bias=bias, q=q, q3=q3, target_ids=target_ids, exclude_ids=excl,
                filt=filt.contiguous(), bw=bw)
