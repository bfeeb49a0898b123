"""Cases and a torch-CPU restatement of the clustered e4m3 scan (csrc/retrieve.hip retr_ivf_q8_topk_k,
retr_rescore_k<true>), shared by tests/test_retrieval_ivf_q8_host.py and tests/test_gpu_retrieval_ivf_q8.py.

Reference: codes and the quantised query are dequantised through float8_e4m3fn (retrieval_q8_case's
quantiser restatement), dots are taken in fp64, the scales are applied, then the prior, eligibility
(tags, exclusion) and the probed-row set; a list is ordered by numpy.lexsort on (id, -score): score
descending, id ascending, the clustered deep call's order.

Integer cases: rows and queries hold integers in -3..3 (amax 1, 2 or 3 per row, so every code is the
integer times a power of two and exact), biases are multiples of 1/4 in [-2, 2] and weights are in
{-1/2, 1/2, 1, 2}.  A dot is an integer of magnitude <= 9 * 128 = 1152 and w * bias a multiple of 1/8 of
magnitude <= 4, so every product, sum and fma is exact in f32 (and in any order): no tolerance, and many
exact ties.  ``int_exact_in_f32`` checks that on the CPU.
"""
import numpy as np
import torch
import torch.nn.functional as F

import retrieval_q8_case as C

D = 128
L = 12
LENGTHS = [250, 0, 1, 63, 64, 65, 129, 1500, 200, 236, 242, 250]  # an empty list, partial tiles, one list > 1024
N = sum(LENGTHS)
_CACHE = {}


def _assignment(seed):
    """int64 [N]: the list of every flat row, a seeded shuffle of the forced lengths."""
    g = torch.Generator().manual_seed(seed)
    assign = torch.cat([torch.full((n,), c, dtype=torch.int64) for c, n in enumerate(LENGTHS)])
    return assign[torch.randperm(N, generator=g)]


def _ids(seed):
    """int64 [N] ascending, distinct, never 0 and never equal to a row number's neighbourhood."""
    g = torch.Generator().manual_seed(seed + 1)
    return torch.cumsum(torch.randint(1, 9, (N,), generator=g), 0) + 100000


def int_case(seed=5):
    """dict: flat ids / items bf16 / tags / bias (id-ascending), assign, centroids bf16 [L, 128], queries
    f32 [65, 128] (integers) and weights f32 [65]."""
    key = ("int", seed)
    if key not in _CACHE:
        g = torch.Generator().manual_seed(seed)
        q, items = C.int_case(65, N, seed=seed)
        tags = torch.randint(0, 16, (N,), generator=g).to(torch.int32)
        bias = (torch.randint(-8, 9, (N,), generator=g).float() / 4).contiguous()
        w = torch.tensor([0.5, 1.0, 2.0, -0.5])[torch.arange(65) % 4].contiguous()
        cen = torch.randn(L, D, generator=g).to(torch.bfloat16)
        _CACHE[key] = dict(ids=_ids(seed), items=items, tags=tags, bias=bias, assign=_assignment(seed), centroids=cen,
                           q=q, w=w)
    return _CACHE[key]


def unit_case(seed=3):
    """The same lists over random unit rows around 16 centres (retrieval_q8_case.unit_case); centroids are
    the normalised list means (a list without rows keeps a random unit vector)."""
    key = ("unit", seed)
    if key not in _CACHE:
        g = torch.Generator().manual_seed(seed)
        q, items = C.unit_case(65, N, True, seed)
        assign = _assignment(seed)
        cen = F.normalize(torch.randn(L, D, generator=g), dim=-1)
        for c in range(L):
            if LENGTHS[c]:
                cen[c] = F.normalize(items[assign == c].float().sum(0), dim=-1)
        tags = torch.randint(0, 16, (N,), generator=g).to(torch.int32)
        bias = (torch.randint(-8, 9, (N,), generator=g).float() / 64).contiguous()
        w = torch.tensor([0.5, 1.0, 2.0, -0.5])[torch.arange(65) % 4].contiguous()
        _CACHE[key] = dict(ids=_ids(seed), items=items, tags=tags, bias=bias, assign=assign,
                           centroids=cen.to(torch.bfloat16), q=q, w=w)
    return _CACHE[key]


def clustered_order(case):
    """(order int64 [N]: the flat row of every clustered row, list_off int64 [L + 1])."""
    order = torch.argsort(case["assign"], stable=True)
    counts = torch.bincount(case["assign"], minlength=L)
    return order, torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(counts, 0)])


def build(case, dev="cpu", tags=True, bias=True):
    """The bf16 ClusteredItemCatalogue of a case on ``dev`` (from_assignment forces the lists)."""
    from recommendations_amd.models.lthm.sequence.retrieval import ClusteredItemCatalogue, ItemCatalogue
    flat = ItemCatalogue(case["ids"], case["items"], case["tags"] if tags else None, case["bias"] if bias else None)
    return ClusteredItemCatalogue.from_assignment(flat.to(dev), case["centroids"].to(dev), case["assign"].to(dev))


def probe_rows(Q, P, seed, all_lists=False):
    """int32 [Q, P]: P distinct lists per query in a seeded order (P = L: every list); query 0 always
    names the empty list 1 first and the long list 7 where P allows."""
    g = torch.Generator().manual_seed(seed)
    out = torch.stack([torch.randperm(L, generator=g)[:P] for _ in range(Q)]).to(torch.int32)
    if not all_lists:
        out[0, 0] = 1
        if P >= 2:
            out[0, 1] = 7
            if P >= 3 and int(out[0, 2]) in (1, 7):
                out[0, 2] = 3
    return out.contiguous()


def approx_f64(case, q_bf):
    """fp64 [Q, N] in the clustered row order: the approximate score of bf16 queries."""
    order, _ = clustered_order(case)
    return C.approx_scores(q_bf, case["items"][order])


def abs_dot_f64(case, q_bf):
    """fp64 [Q, N]: sum_k |a_k b_k| of the dequantised operands, clustered order (the error bound's scale)."""
    order, _ = clustered_order(case)
    cq, sq, _ = C.quantize_ref(q_bf)
    ci, si, _ = C.quantize_ref(case["items"][order])
    return (C.dequant(cq, sq).abs() @ C.dequant(ci, si).abs().T).numpy()


def eligible(case, probes, excl_rows=None, filt=None):
    """bool [Q, N], clustered order: the row lies in a probed list, is not excluded and passes the filter."""
    order, off = clustered_order(case)
    Q = probes.shape[0]
    ok = np.zeros((Q, N), dtype=bool)
    for i in range(Q):
        for c in probes[i].tolist():
            if 0 <= c < L:
                ok[i, int(off[c]):int(off[c + 1])] = True
    if excl_rows is not None:
        for i, lst in enumerate(excl_rows.tolist()):
            for r in lst:
                if 0 <= r < N:
                    ok[i, r] = False
    if filt is not None:
        t = case["tags"][order].numpy().astype(np.int64)
        for i in range(Q):
            fa, fy, fn = (int(v) for v in filt[i])
            passes = ((t & fa) == fa) & ((t & fn) == 0) & (((t & fy) != 0) if fy else True)
            ok[i] &= passes
    return ok


def ranked_scores(case, s64, w=None):
    """The ranked score of every (query, clustered row): s64 as f32, and with weights w f32 [Q] the prior
    added by torch.addcmul in f32 on the f32-rounded score."""
    order, _ = clustered_order(case)
    s = torch.from_numpy(s64).float()
    if w is not None:
        s = torch.addcmul(s, w[:, None].float(), case["bias"][order][None, :].float())
    return s.numpy()


def first_m(case, s, ok, M):
    """(scores f32 [Q, M], rows int32 [Q, M]) of ranked scores s [Q, N] and eligibility ok: the M first
    under (score descending, id ascending), then (-inf, -1).  Rows are clustered rows."""
    order, _ = clustered_order(case)
    ids = case["ids"][order].numpy()
    Q = s.shape[0]
    rows = np.full((Q, M), -1, dtype=np.int32)
    sc = np.full((Q, M), -np.inf, dtype=np.float32)
    for i in range(Q):
        cand = np.nonzero(ok[i])[0]
        o = cand[np.lexsort((ids[cand], -s[i, cand].astype(np.float64)))][:M]
        rows[i, :len(o)] = o
        sc[i, :len(o)] = s[i, o]
    return sc, rows


def int_exact_in_f32(case):
    """The integer case's scores and fmas are exact in f32: the fp64 values survive the round trip, and
    the fp64 prior equals the f32 addcmul."""
    q_bf = case["q"].to(torch.bfloat16)
    assert torch.equal(q_bf.float(), case["q"])
    s64 = approx_f64(case, q_bf)
    assert np.array_equal(s64.astype(np.float32).astype(np.float64), s64)
    assert np.abs(s64).max() <= 9 * D and np.array_equal(s64, np.round(s64))
    order, _ = clustered_order(case)
    want = s64 + case["w"].double().numpy()[:, None] * case["bias"][order].double().numpy()[None, :]
    got = ranked_scores(case, s64, case["w"])
    assert np.array_equal(got.astype(np.float64), want)
    exact = C.exact_scores(q_bf, case["items"][order])
    assert np.array_equal(exact, s64)  # every code is exact, so the approximate score is the exact one
    return True
