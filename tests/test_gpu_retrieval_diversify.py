"""Diversified lists on the GPU (csrc/retrieve.hip retr_diversify_k, lthm_retrieve_diversify,
K.retrieve_diversify, torch.ops.lthm.retrieve_diversify, ItemCatalogue.diversify,
LTHMModelWrapper.retrieve(diversity=, group_cap=)).

Exact cases (tests/retrieval_diversify_case.py: rows in {-2..2}, integer scores, lam in {0, 0.5, 1})
are compared bit for bit against the fp64 greedy: every product and sum there is an integer or a half
below 2^24, so every f32 evaluation order gives the same value.  Objectives are compared after + 0
(the contract orders -0 and +0 as equal, and lam = 0 gives -0 d).  Unit-vector cases are checked along
the kernel's own path (follow) with eps = 2e-5: an f32 dot of 128 products of unit vectors errs by at
most 128 * 2^-24 * sum|a_i b_i| <= 7.7e-6, on both compared objectives, weighted lam and 1 - lam."""
import numpy as np
import pytest
import torch

from retrieval_diversify_case import D, EPS, EXACT_N, exact_items, exact_pool, follow, greedy

pytestmark = pytest.mark.gpu

_CACHE = {}


def bits(t):
    return (t.contiguous().cpu() + 0.0).view(torch.int32)


def _items(dev):
    if "exact" not in _CACHE:
        emb, groups = exact_items()
        _CACHE["exact"] = (emb, groups, emb.to(dev), groups.to(dev))
    return _CACHE["exact"]


def _same(got, want, what):
    r, s, o = (x.cpu() for x in got)
    assert torch.equal(r, torch.from_numpy(want[0])), what
    assert torch.equal(bits(s), bits(torch.from_numpy(want[1]))), what
    assert torch.equal(bits(o), bits(torch.from_numpy(want[2]))), what


@pytest.mark.parametrize("M", [1, 63, 64, 65, 257, 1024])
def test_exact_pools_bit_equal_to_the_checker(dev, M):
    """Q = 5 pools of different live length (padding rows -1 and N, -inf and NaN scores, a query with
    no candidate), lam = (1, 0.5, 0, 0.5, 1) per query, k in {1, 10, 128} (k > M leaves empties), with
    and without groups (cap 2)."""
    from recommendations_amd import kernels as K
    emb, groups, emb_d, groups_d = _items(dev)
    rows, scores, lam = exact_pool(M)
    rows_d, scores_d, lam_d = rows.to(dev), scores.to(dev), lam.to(dev)
    for k in (1, 10, 128):
        got = K.retrieve_diversify(emb_d, rows_d, scores_d, k, lam=lam_d)
        _same(got, greedy(rows, scores, emb, k, lam), (M, k))
        assert bool((got[0][3] == -1).all()) and bool(torch.isneginf(got[1][3]).all()) and bool(torch.isneginf(got[2][3]).all())
        if k > M:
            assert bool((got[0][:, M:] == -1).all())
        got = K.retrieve_diversify(emb_d, rows_d, scores_d, k, lam=lam_d, groups=groups_d, cap=2)
        _same(got, greedy(rows, scores, emb, k, lam, groups, 2), (M, k, "cap"))
    # lam = None is 1 everywhere
    got = K.retrieve_diversify(emb_d, rows_d, scores_d, 10)
    _same(got, greedy(rows, scores, emb, 10), (M, "lam None"))
    assert torch.equal(bits(got[1]), bits(got[2]))  # m = s bit for bit


def test_shuffled_pool_at_lam_1_is_the_scan_s_own_first_k(dev):
    """The identity: lam = 1 without groups returns the first k of the pool under (score descending,
    row ascending) whatever order the pool came in, which is what K.retrieve_topk itself returns."""
    from recommendations_amd import kernels as K
    emb, _, emb_d, _ = _items(dev)
    g = torch.Generator().manual_seed(31)
    q = torch.randint(-2, 3, (5, D), generator=g).float().to(dev)
    for M, k in ((300, 128), (1024, 100), (128, 128)):
        sc, rw, _, _ = K.retrieve_topk(q, emb_d, M, normalize_q=False, deep=M > K.RETRIEVE_MAX_K)
        perm = torch.stack([torch.randperm(M, generator=g) for _ in range(5)]).to(dev)
        got = K.retrieve_diversify(emb_d, rw.gather(1, perm).contiguous(), sc.gather(1, perm).contiguous(), k)
        assert torch.equal(got[0], rw[:, :k]), (M, k)
        assert torch.equal(bits(got[1]), bits(sc[:, :k])) and torch.equal(bits(got[2]), bits(sc[:, :k]))


def test_caps(dev):
    """cap in {1, 2}; one key owning more than k candidates; key 0 never capped; exhaustion with fewer
    than k eligible; the tie on the objective going to the lower row."""
    from recommendations_amd import kernels as K
    emb, _, emb_d, _ = _items(dev)
    N, M, k = EXACT_N, 300, 10
    g = torch.Generator().manual_seed(77)
    rows = torch.stack([torch.randperm(N, generator=g)[:M] for _ in range(3)]).to(torch.int32)
    scores = torch.randint(0, 3, (3, M), generator=g).float()
    lam = torch.tensor([1.0, 0.5, 1.0])
    # key 9 owns most rows, key 0 every seventh, keys 1..3 a few
    groups = torch.full((N,), 9, dtype=torch.int32)
    groups[::7] = 0
    groups[3::50] = 1
    groups[4::50] = 2
    groups[5::50] = 3
    for cap in (1, 2):
        got = K.retrieve_diversify(emb_d, rows.to(dev), scores.to(dev), k, lam=lam.to(dev), groups=groups.to(dev), cap=cap)
        _same(got, greedy(rows, scores, emb, k, lam, groups, cap), cap)
        keys = groups[got[0].cpu().long()]
        assert bool((got[0] >= 0).all())
        for key in (1, 2, 3, 9):
            assert bool(((keys == key).sum(dim=1) <= cap).all()), (cap, key)
        assert bool(((keys == 0).sum(dim=1) >= k - 4 * cap).all())  # key 0 fills what the caps leave free
    # exhaustion: no key 0, four keys, cap 2: eight items and two empty slots
    nz = groups.clone()
    nz[::7] = 9
    got = K.retrieve_diversify(emb_d, rows.to(dev), scores.to(dev), k, lam=lam.to(dev), groups=nz.to(dev), cap=2)
    _same(got, greedy(rows, scores, emb, k, lam, nz, 2), "exhaustion")
    assert bool((got[0][:, :5] >= 0).all()) and bool((got[0][:, 8:] == -1).all()) and bool(torch.isneginf(got[2][:, 8:]).all())
    # ties: equal scores at lam = 1, so the rows come ascending, each key's cap permitting
    flat_scores = torch.ones((3, M))
    got = K.retrieve_diversify(emb_d, rows.to(dev), flat_scores.to(dev), k, groups=groups.to(dev), cap=1)
    _same(got, greedy(rows, flat_scores, emb, k, None, groups, 1), "ties")
    for qi in range(3):
        order = torch.sort(rows[qi])[0]
        want, seen = [], set()
        for r in order.tolist():
            key = int(groups[r])
            if key == 0 or key not in seen:
                want.append(r)
                seen.add(key)
        assert got[0][qi].cpu().tolist() == want[:k]
    # a row named twice is two candidates, the lower position first, and stays memory-safe
    twice = torch.tensor([[5, 9, 5, 9, N + 3, -2]], dtype=torch.int32)
    sc = torch.tensor([[1.0, 2.0, 1.0, 2.0, 9.0, 9.0]])
    got = K.retrieve_diversify(emb_d, twice.to(dev), sc.to(dev), 6)
    _same(got, greedy(twice, sc, emb, 6), "twice")
    assert got[0].cpu().tolist() == [[9, 9, 5, 5, -1, -1]]


def _unit(dev):
    if "unit" not in _CACHE:
        from recommendations_amd import kernels as K
        from retrieval_ivf_case import unit_case
        c = unit_case(4096, 50, 8, 123)
        emb_d = c["emb"].to(dev)
        groups = c["assign"].to(torch.int32)  # the centre an item was drawn around; key 0 (centre 0) is never capped
        pools = {}
        for M in (300, 1024):
            sc, rw, _, _ = K.retrieve_topk(c["q"].to(dev), emb_d, M, normalize_q=False, deep=True)
            pools[M] = (rw.contiguous(), sc.contiguous())
        _CACHE["unit"] = (c["emb"], emb_d, groups, pools)
    return _CACHE["unit"]


@pytest.mark.parametrize("M", [300, 1024])
@pytest.mark.parametrize("cap", [None, 3])
def test_unit_vectors_follow_the_contract(dev, M, cap):
    """N = 4,096 unit rows around 50 centres, Q = 8, k = 100, lam per query in {0.3, 0.7}; the pool is
    the deep scan's own list."""
    from recommendations_amd import kernels as K
    emb, emb_d, groups, pools = _unit(dev)
    rw, sc = pools[M]
    lam = torch.tensor([0.3, 0.7] * 4)
    got = K.retrieve_diversify(emb_d, rw, sc, 100, lam=lam.to(dev), groups=None if cap is None else groups.to(dev),
                               cap=cap or 1)
    follow(rw, sc, emb, got[0], got[1], got[2], lam, None if cap is None else groups, cap or 1, EPS)
    if cap is None:
        assert bool((got[0] >= 0).all())
    else:  # a query's best candidates share its centre's key: the cap binds
        keys = groups[got[0].cpu().clamp(min=0).long()]
        assert bool((((keys == keys[:, :1]) & (keys != 0)).sum(dim=1) <= cap).all())
    # diversity does something: the list differs from the first 100 by score
    assert not torch.equal(got[0], rw[:, :100])


def test_script_op(dev):
    from recommendations_amd import _lib
    from recommendations_amd import kernels as K
    _lib.load_torch_ops()
    emb, groups, emb_d, groups_d = _items(dev)
    rows, scores, lam = exact_pool(257)
    rows_d, scores_d, lam_d = rows.to(dev), scores.to(dev), lam.to(dev)

    @torch.jit.script
    def run(items: torch.Tensor, r: torch.Tensor, s: torch.Tensor, k: int, lam_: torch.Tensor, groups_: torch.Tensor, cap: int):
        return torch.ops.lthm.retrieve_diversify(items, r, s, k, lam_, groups_, cap)

    want = K.retrieve_diversify(emb_d, rows_d, scores_d, 10, lam=lam_d, groups=groups_d, cap=2)
    for got in (run(emb_d, rows_d, scores_d, 10, lam_d, groups_d, 2),
                torch.ops.lthm.retrieve_diversify(emb_d, rows_d, scores_d, 10, lam_d, groups_d, 2)):
        for a, b in zip(got, want):
            assert torch.equal(a, b)
    got = torch.ops.lthm.retrieve_diversify(emb_d, rows_d, scores_d, 10)
    for a, b in zip(got, K.retrieve_diversify(emb_d, rows_d, scores_d, 10)):
        assert torch.equal(a, b)
    with pytest.raises(RuntimeError, match=r"takes a pool of 1\.\.1024 candidates \(got M=1025\)"):
        torch.ops.lthm.retrieve_diversify(emb_d, torch.zeros((1, 1025), dtype=torch.int32, device=dev),
                                          torch.zeros((1, 1025), device=dev), 5)
    with pytest.raises(RuntimeError, match=r"takes a pool of 1\.\.1024 candidates \(got M=1025\)"):
        K.retrieve_diversify(emb_d, torch.zeros((1, 1025), dtype=torch.int32, device=dev), torch.zeros((1, 1025), device=dev), 5)
    with pytest.raises(RuntimeError, match=r"takes k in 1\.\.128 \(got 129\)"):
        K.retrieve_diversify(emb_d, rows_d, scores_d, 129)


def test_catalogue_diversify_maps_ids(dev):
    """ItemCatalogue.diversify: ids the catalogue does not hold and the pad id 0 are no candidates,
    empty slots come back as id 0."""
    from recommendations_amd.models.lthm.sequence.retrieval import ItemCatalogue
    emb, groups, emb_d, groups_d = _items(dev)
    ids = torch.arange(1, EXACT_N + 1, dtype=torch.int64) * 5 + 2
    cat = ItemCatalogue(ids.to(dev), emb_d, None, None, groups_d)
    rows, scores, _ = exact_pool(65, seed=3)
    rows, scores = rows[:1].clone(), scores[:1].clone()
    pool_ids = ids[rows.long()].clone()
    pool_ids[0, ::4] = 0            # the pad id
    pool_ids[0, 1::4] = 4           # below every id, held by nobody
    pool_ids[0, 2::8] = 1 << 50     # above every id
    live_rows = cat.rows_of(pool_ids.to(dev)).cpu()
    assert int((live_rows >= 0).sum()) == 65 - 17 - 16 - 8
    for lam, cap in ((1.0, None), (0.5, None), (0.5, 1), (torch.tensor([0.0]), 2)):
        got = cat.diversify(pool_ids.to(dev), scores.to(dev), 40, lam=lam, group_cap=cap)
        lam_t = lam if isinstance(lam, torch.Tensor) else torch.tensor([lam])
        want = greedy(live_rows, scores, emb, 40, lam_t, None if cap is None else groups, cap or 1)
        want_ids = np.where(want[0] >= 0, ids.numpy()[np.maximum(want[0], 0)], 0)
        assert torch.equal(got[0].cpu(), torch.from_numpy(want_ids)), (lam, cap)
        assert torch.equal(bits(got[1]), bits(torch.from_numpy(want[1]))) and torch.equal(bits(got[2]), bits(torch.from_numpy(want[2])))
        assert got[0].dtype == torch.int64 and bool((got[0][0, 24:] == 0).all())


def test_wrapper_retrieve_diversified(dev):
    """LTHMModelWrapper.retrieve(diversity=, group_cap=) on the smallest configuration of
    tests/test_gpu_wrapper_api.py: its result is ItemCatalogue.diversify applied to the same call's
    pool, bit for bit, and it composes with exclude_history."""
    from recommendations_amd.data import synthetic_lthm_batch
    from recommendations_amd.models.lthm.config import lthm_config
    from recommendations_amd.models.lthm.sequence.retrieval import build_catalogue
    from recommendations_amd.models.lthm.sequence.wrapper import LTHMModelWrapper
    torch.manual_seed(0)
    cfg = lthm_config(T=30, d=64, n_layers=1, n_head=2, item_vocab=1000, lookahead=[0, 2, 4], out_emb_dim=D,
                      gradient_checkpointing=False)
    m = LTHMModelWrapper(cfg).to(dev).eval()
    batch = synthetic_lthm_batch(20, 30, seed=3, device=dev)
    ids = batch["product_ids"].reshape(-1)
    extra = torch.randint(1, 2 ** 62, (300,), generator=torch.Generator().manual_seed(5)).to(dev)
    all_ids = torch.cat([extra, ids[ids != 0]])
    cat = build_catalogue(m, all_ids, chunk=128, groups=(all_ids % 6).to(torch.int32))
    assert cat.has_groups and torch.equal(cat.groups, (cat.ids % 6).to(torch.int32))
    for kw, lam, cap, pool in ((dict(diversity=0.6), 0.6, None, 160), (dict(group_cap=2), 1.0, 2, 160),
                               (dict(diversity=0.4, group_cap=1, pool=200, exclude_history=True), 0.4, 1, 200),
                               (dict(diversity=0.5, pool=64, heads=[0, 2]), 0.5, None, 64)):
        got = m.retrieve(batch, cat, 20, **kw)
        base = {n: v for n, v in kw.items() if n in ("exclude_history", "heads")}
        pl = m.retrieve(batch, cat, pool, **base)
        want = cat.diversify(pl["item_ids"], pl["scores"], 20, lam=lam, group_cap=cap)
        assert torch.equal(got["item_ids"], want[0]), kw
        assert torch.equal(got["scores"].view(torch.int32), want[1].view(torch.int32)), kw
        assert torch.equal(got["objective"].view(torch.int32), want[2].view(torch.int32)), kw
        if cap is not None:
            keys = got["item_ids"] % 6
            for key in range(1, 6):
                assert bool((((keys == key) & (got["item_ids"] != 0)).sum(dim=1) <= cap).all()), (kw, key)
        if kw.get("exclude_history"):
            seen = batch["product_ids"]
            assert not bool((got["item_ids"][:, :, None] == seen[:, None, :]).logical_and(got["item_ids"][:, :, None] != 0).any())
    assert set(m.retrieve(batch, cat, 20)) == {"item_ids", "scores"}  # the plain call is what it was
