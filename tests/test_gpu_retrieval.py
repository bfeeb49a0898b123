"""Full-catalogue top-K retrieval (csrc/retrieve.hip, K.retrieve_topk, ItemCatalogue,
LTHMModelWrapper.retrieve / catalogue_metrics) against a checker written here.

The reference has no retrieval code, so the checker is torch on the CPU in fp64 over the same
bf16-rounded operands, ordered by numpy.lexsort on (row, -score): score descending, row
ascending (torch.topk's tie order is unspecified).

Exact cases: integer operands in {-2..2}, normalize_q=False; every partial sum is an integer
below 2^10, so every summation order gives the same f32 and scores / rows / rank must match
bit for bit.  The catalogue holds 1,367 random rows three times each at permuted positions
(N = 4,101), which puts score ties at every rank.

Normalised cases: unit-vector operands, normalize_q=True on f32 queries, eps = 1e-5.  f32
accumulation of 128 products errs by at most 128 * 2^-24 * sum|a_i b_i| <= 7.7e-6 for unit
vectors.  The queries' f32 values are bf16-representable, so re-normalising them (norm within
2e-4 of 1, far inside half a bf16 ulp) rounds back to the same bf16 whatever order the norm
is summed in: the checker and the kernel see the same operands.
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from lthm_step_case import build_wrapper, load_case
from parity import check, relerr

pytestmark = pytest.mark.gpu

EPS = 1e-5
D = 128
_CACHE = {}


# ------------------------------------------------------------------ checker (CPU, fp64)
def checker(q_bf, items_bf, k, trow=None):
    """q_bf [Q, 128], items_bf [N, 128]: the bf16 operands.  Returns fp64 scores [Q, N], the
    expected (scores f32 [Q, k], rows int32 [Q, k]) and rank int32 [Q] (or None)."""
    s = (q_bf.double() @ items_bf.double().T).numpy()
    Q, N = s.shape
    rows = np.full((Q, k), -1, dtype=np.int32)
    sc = np.full((Q, k), -np.inf, dtype=np.float32)
    ar = np.arange(N)
    for i in range(Q):
        order = np.lexsort((ar, -s[i]))[:k]
        rows[i, :len(order)] = order
        sc[i, :len(order)] = s[i, order].astype(np.float32)
    rank = None
    if trow is not None:
        rank = np.full(Q, -1, dtype=np.int32)
        for i in range(Q):
            t = int(trow[i])
            if t >= 0:
                rank[i] = int((s[i] > s[i, t]).sum())  # strict: the target itself never counts
    return s, sc, rows, rank


def int_catalogue():
    if "int" not in _CACHE:
        g = torch.Generator().manual_seed(1234)
        base = torch.randint(-2, 3, (1367, D), generator=g)
        perm = torch.randperm(3 * 1367, generator=g)
        items = base.repeat(3, 1)[perm].to(torch.bfloat16)
        q = torch.randint(-2, 3, (70, D), generator=g).float()
        _CACHE["int"] = (q, items)
    return _CACHE["int"]


def run_exact(dev, q, items, k, slab_rows, with_target=True):
    from recommendations_amd import kernels as K
    Q, N = q.shape[0], items.shape[0]
    trow = None
    if with_target:
        trow = ((torch.arange(Q) * 7919 + 3) % N).to(torch.int32)
        trow[::5] = -1
    s, e_sc, e_rows, e_rank = checker(q.to(torch.bfloat16), items, k, None if trow is None else trow.numpy())
    scores, rows, rank, tscore = K.retrieve_topk(q.to(dev), items.to(dev), k, normalize_q=False,
                                                 target_rows=None if trow is None else trow.to(dev),
                                                 slab_rows=slab_rows)
    assert np.array_equal(rows.cpu().numpy(), e_rows), (Q, N, k, slab_rows)
    assert np.array_equal(scores.cpu().numpy().view(np.uint32), e_sc.view(np.uint32)), (Q, N, k, slab_rows)
    if with_target:
        assert np.array_equal(rank.cpu().numpy(), e_rank), (Q, N, k, slab_rows)
        ts = tscore.cpu().numpy()
        for i in range(Q):
            if trow[i] >= 0:
                assert ts[i] == np.float32(s[i, int(trow[i])])
    return scores, rows, rank


@pytest.mark.parametrize("slabs", ["auto", "min"])
@pytest.mark.parametrize("Q,N,k", [(33, 4101, 10), (1, 4101, 1), (70, 4101, 128), (5, 7, 10), (33, 63, 64)])
def test_exact_integer_cases(dev, Q, N, k, slabs):
    from recommendations_amd import kernels as K
    q, items = int_catalogue()
    run_exact(dev, q[:Q].contiguous(), items[:N].contiguous(), k, 0 if slabs == "auto" else K.RETRIEVE_MIN_SLAB_ROWS)


@pytest.mark.parametrize("descending", [False, True])
def test_filter_worst_case(dev, descending):
    """Query 0's scores ascend with the row: every item passes the threshold and the prune runs
    at every tile.  And the opposite order."""
    q, items = int_catalogue()
    s0 = items.double() @ q[0].double()
    order = torch.argsort(s0, stable=True, descending=descending)
    run_exact(dev, q[:33].contiguous(), items[order].contiguous(), 100, 0)


@pytest.mark.parametrize("place", ["first", "last", "straddle"])
def test_best_item_placement(dev, place):
    from recommendations_amd import kernels as K
    q, items = int_catalogue()
    q = q[:33].clone()
    q[0][q[0] == 0] = 1.0
    items = items.clone()
    best = (2 * torch.sign(q[0])).to(torch.bfloat16)  # the largest score any item can reach on query 0
    second = best.clone()
    second[0] = -second[0]
    N = items.shape[0]
    slab = K.RETRIEVE_MIN_SLAB_ROWS
    if place == "first":
        items[0] = best
    elif place == "last":
        assert N % 64 != 0  # the last row lies in a partial tile
        items[N - 1] = best
    else:
        items[slab - 1] = best
        items[slab] = second
    _, rows, _ = run_exact(dev, q, items, 10, slab if place == "straddle" else 0)
    want = {"first": [0], "last": [N - 1], "straddle": [slab - 1, slab]}[place]
    assert rows[0, :len(want)].tolist() == want


# ------------------------------------------------------------------ normalised operands
def unit_case(Q, N, clustered, seed):
    key = ("unit", Q, N, clustered, seed)
    if key not in _CACHE:
        g = torch.Generator().manual_seed(seed)
        if clustered:
            centres = F.normalize(torch.randn(50, D, generator=g), dim=-1)
            x = centres[torch.randint(0, 50, (N,), generator=g)] + 0.05 * torch.randn(N, D, generator=g)
        else:
            x = torch.randn(N, D, generator=g)
        items = F.normalize(x, dim=-1).to(torch.bfloat16)
        q = F.normalize(torch.randn(Q, D, generator=g), dim=-1).to(torch.bfloat16).float()
        # the bf16 operand the kernel forms from q is q itself (module docstring)
        assert torch.equal(F.normalize(q, dim=-1).to(torch.bfloat16).float(), q)
        _CACHE[key] = (q, items)
    return _CACHE[key]


def check_eps_rules(s, k, g_scores, g_rows, trow=None, g_rank=None):
    """The eps rules of the normalised cases, per query, on fp64 scores s [Q, N]."""
    Q, N = s.shape
    kk = min(k, N)
    for i in range(Q):
        kth = np.sort(s[i])[::-1][kk - 1]
        # condition on the checker's own scores, before the GPU's are looked at
        assert int((np.abs(s[i] - kth) <= EPS).sum()) <= 4, "too many catalogue rows within eps of the k-th score"
    for i in range(Q):
        kth = np.sort(s[i])[::-1][kk - 1]
        r = g_rows[i, :kk]
        assert (r >= 0).all() and (r < N).all() and len(set(r.tolist())) == kk
        assert (g_rows[i, kk:] == -1).all()
        assert np.abs(g_scores[i, :kk].astype(np.float64) - s[i, r]).max() <= EPS
        must = np.nonzero(s[i] > kth + EPS)[0]
        assert set(must.tolist()) <= set(r.tolist())
        assert (s[i, r] >= kth - EPS).all()
        assert (np.diff(g_scores[i, :kk]) <= 0).all()
        if trow is not None and trow[i] >= 0:
            t = int(trow[i])
            others = np.delete(s[i], t)
            lo, hi = int((others > s[i, t] + EPS).sum()), int((others >= s[i, t] - EPS).sum())
            assert lo <= int(g_rank[i]) <= hi, (i, lo, int(g_rank[i]), hi)
        elif trow is not None:
            assert int(g_rank[i]) == -1


@pytest.mark.parametrize("Q,N,k,clustered", [(70, 5000, 100, False), (33, 4099, 10, False), (70, 5000, 100, True),
                                             (33, 4099, 10, True)])
def test_normalised_random(dev, Q, N, k, clustered):
    from recommendations_amd import kernels as K
    q, items = unit_case(Q, N, clustered, 7 + Q)
    trow = ((torch.arange(Q) * 104729 + 11) % N).to(torch.int32)
    trow[3::7] = -1
    s = (q.double() @ items.double().T).numpy()
    scores, rows, rank, _ = K.retrieve_topk(q.to(dev), items.to(dev), k, normalize_q=True, target_rows=trow.to(dev))
    check_eps_rules(s, k, scores.cpu().numpy(), rows.cpu().numpy(), trow.numpy(), rank.cpu().numpy())


def test_bf16_queries_match_f32(dev):
    from recommendations_amd import kernels as K
    q, items = unit_case(33, 4099, False, 40)
    a = K.retrieve_topk(q.to(dev), items.to(dev), 10, normalize_q=False)
    b = K.retrieve_topk(q.to(torch.bfloat16).to(dev), items.to(dev), 10, normalize_q=False)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_deterministic(dev):
    from recommendations_amd import kernels as K
    q, items = unit_case(70, 5000, True, 77)
    trow = (torch.arange(70) % 5000).to(torch.int32).to(dev)
    qd, it = q.to(dev), items.to(dev)
    a = K.retrieve_topk(qd, it, 100, target_rows=trow)
    b = K.retrieve_topk(qd, it, 100, target_rows=trow)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


# ------------------------------------------------------------------ refusals
def test_refusals(dev):
    from recommendations_amd import _lib
    from recommendations_amd import kernels as K
    q = torch.zeros((4, D), device=dev)
    items = torch.zeros((100, D), dtype=torch.bfloat16, device=dev)
    for bad_k in (0, 129):
        with pytest.raises(RuntimeError):
            K.retrieve_topk(q, items, bad_k)
    with pytest.raises(RuntimeError):
        K.retrieve_topk(q, items[:0], 5)
    with pytest.raises(RuntimeError):
        K.retrieve_topk(q[:, :64].contiguous(), torch.zeros((100, 64), dtype=torch.bfloat16, device=dev), 5)
    with pytest.raises(RuntimeError):
        K.retrieve_topk(q, items, 5, slab_rows=100)
    with pytest.raises(RuntimeError, match="MI355X"):
        K.retrieve_topk(q.cpu(), items.cpu(), 5)
    # a too-small workspace through the raw ABI: refused before any launch
    lib = _lib.load()
    need = lib.lthm_retrieve_ws_bytes(4, 100, 5, 0)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    scores = torch.full((4, 5), 123.0, device=dev)
    rows = torch.full((4, 5), 77, dtype=torch.int32, device=dev)
    d = _lib.STRUCTS["lthm_retrieve_desc"]()
    d.items, d.q, d.scores, d.rows = items.data_ptr(), q.data_ptr(), scores.data_ptr(), rows.data_ptr()
    d.workspace, d.ws_bytes = ws.data_ptr(), need - 1
    d.Q, d.N, d.k, d.q_dtype, d.normalize_q, d.slab_rows = 4, 100, 5, _lib.F32, 1, 0
    stream = torch.cuda.current_stream().cuda_stream
    assert lib.lthm_retrieve_topk(ctypes.addressof(d), stream) != 0
    torch.cuda.synchronize()
    assert bool((scores == 123.0).all()) and bool((rows == 77).all())
    d.ws_bytes = need
    d.items = items.data_ptr() + 2  # 16-byte alignment of the catalogue
    assert lib.lthm_retrieve_topk(ctypes.addressof(d), stream) != 0
    d.items = items.data_ptr()
    assert lib.lthm_retrieve_topk(ctypes.addressof(d), stream) == 0
    torch.cuda.synchronize()
    assert bool((rows[:, 0] == 0).all())  # all scores tie at 0: row ascending


# ------------------------------------------------------------------ model level
def _model_case(dev):
    if "model" not in _CACHE:
        from recommendations_amd.models.lthm.sequence.retrieval import build_catalogue
        fx, params, _, batch = load_case("lthm_step_a")
        m = build_wrapper(fx, params, dev).eval()
        b = {k: v.to(dev) for k, v in batch.items()}
        with torch.no_grad():
            out = m(b)
        ids = batch["product_ids"].reshape(-1)
        g = torch.Generator().manual_seed(5)
        extra = torch.randint(1, 2 ** 62, (300,), generator=g)
        cat_ids = torch.cat([extra, ids[ids != 0]])  # unsorted, with repeats: build_catalogue sorts
        assert bool(torch.isin(ids[ids != 0], cat_ids).all())
        cat = build_catalogue(m, cat_ids, chunk=128)  # several chunks
        _CACHE["model"] = (m, b, out, cat)
    return _CACHE["model"]


def test_build_catalogue_matches_forward(dev):
    m, b, out, cat = _model_case(dev)
    ids = out["current_token_ids"].reshape(-1)
    keep = (out["current_token_mask"].reshape(-1) == 0).cpu()
    want = F.normalize(out["current_token_emb"].float().reshape(-1, D), dim=-1).cpu()[keep]
    rows = cat.rows_of(ids).cpu()[keep]
    assert (rows >= 0).all()
    got = cat.emb.float().cpu()[rows.long()]
    check("catalogue rows vs normalised current_token_emb", relerr(got, want), 7e-3)
    assert 250 <= len(cat) <= 400 and cat.emb.dtype == torch.bfloat16


def test_wrapper_retrieve_matches_checker(dev):
    m, b, out, cat = _model_case(dev)
    k = 20
    res = m.retrieve(b, cat, k)
    assert res["item_ids"].dtype == torch.int64 and res["item_ids"].shape == (b["product_ids"].shape[0], k)
    q_bf = F.normalize(out["next_token_emb"][:, -1, 0].float().cpu(), dim=-1).to(torch.bfloat16)
    s = (q_bf.double() @ cat.emb.cpu().double().T).numpy()
    g_rows = cat.rows_of(res["item_ids"]).cpu().numpy()
    check_eps_rules(s, k, res["scores"].cpu().numpy(), g_rows)
    assert torch.equal(cat.ids[torch.from_numpy(g_rows).long().to(dev)], res["item_ids"])


def test_catalogue_metrics_match_checker(dev):
    m, b, out, cat = _model_case(dev)
    head, ks = 1, [1, 5, 20]
    off = m._lookahead[head]
    ids = out["current_token_ids"].cpu()
    mask = out["current_token_mask"].cpu()
    L = ids.shape[1] - off
    keep = mask[:, off:] == 0
    trow = cat.rows_of(ids[:, off:]).cpu()[keep].numpy()
    assert (trow >= 0).all() and len(trow) > 10
    q_bf = F.normalize(out["next_token_emb"][:, :L, head].float().cpu()[keep], dim=-1).to(torch.bfloat16)
    s = (q_bf.double() @ cat.emb.cpu().double().T).numpy()
    n = len(trow)
    ts = s[np.arange(n), trow]
    lo = (s > ts[:, None] + EPS).sum(1)
    hi = (s >= ts[:, None] - EPS).sum(1) - 1  # without the target itself
    # the checker's rank of a target is certain up to the items within eps of it: lo <= rank <= hi.
    # Every metric is monotone in the ranks, so it lies between its values at lo and at hi
    # (equal to the checker's own where lo == hi).
    assert (lo <= hi).all()
    got = m.catalogue_metrics(out, cat, ks=ks, head=head)
    assert got["catalogue_queries"] == n
    p_lo, p_hi = torch.from_numpy(lo.astype(np.float32)), torch.from_numpy(hi.astype(np.float32))
    tol = 1e-6
    for k in ks:
        v = got[f"hit_rate_at_{k}_catalogue"]
        assert float((p_hi < k).float().mean()) - tol <= v <= float((p_lo < k).float().mean()) + tol, (k, v)
    for key, fn in (("average_hit_position_catalogue", lambda p: float(p.mean())),
                    ("median_hit_position_catalogue", lambda p: float(p.quantile(q=0.5)))):
        assert fn(p_lo) * (1 - tol) - tol <= got[key] <= fn(p_hi) * (1 + tol) + tol, (key, got[key], fn(p_lo), fn(p_hi))
    print("catalogue metrics", got, "uncertain ranks", int((lo != hi).sum()), "of", n)
