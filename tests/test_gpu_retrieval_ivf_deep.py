"""Deep lists on clustered catalogues, on the GPU (csrc/retrieve.hip retr_ivf_deep_topk_k,
lthm_retrieve_ivf_topk_deep, K.retrieve_ivf_topk(deep=True), torch.ops.lthm.retrieve_ivf_topk_deep,
ClusteredItemCatalogue.with_deep(), LTHMModelWrapper.retrieve on the view).

The contract: per query, bit for bit, the k <= 1,024 first under (score descending, id ascending) of the
items that lie in the probed lists, are not excluded, pass the tag filter and lie strictly behind the
cursor, then (-inf, 0); every score the f32 the flat scan returns for the same (query, item, weight).
Exact cases (tests/retrieval_ivf_deep_case.py) are compared bit for bit against two oracles:
  A  the flat ItemCatalogue's deep list with the same arguments, restricted to the probed lists through
     the high tag bits (`none` gains 1 << (16 + list) of every list the query does not probe);
  B  the fp64 checker of retrieval_ivf_filt_case.py.
Unit-vector data is compared GPU against GPU, bit for bit.  Nothing is tolerated anywhere.
"""
import ctypes

import numpy as np
import pytest
import torch

from retrieval_diversify_case import exact_items, exact_pool, greedy
from retrieval_ivf_case import D, spread_ids, unit_case
from retrieval_ivf_deep_case import (DEEP_KS, DEEP_Q, LONG, deep_case, deep_exclude, exact_bias, ivf_filt_checker,
                                     restrict_to_probes, shape_cursors, shape_filters, shape_weights, user_tags)

pytestmark = pytest.mark.gpu

_CACHE = {}


def bits(t):
    return t.contiguous().view(torch.int32)


def _same(got, want, what):
    assert torch.equal(got[1].cpu(), want[1].cpu()), what
    assert torch.equal(bits(got[0].cpu()), bits(want[0].cpu())), what


def _catalogues(c, tags, bias, dev):
    """(flat ItemCatalogue, its with_deep() clustered view) on the device."""
    from recommendations_amd.models.lthm.sequence.retrieval import ClusteredItemCatalogue, ItemCatalogue
    flat = ItemCatalogue(c["ids"].to(dev), c["emb"].to(dev), tags.to(dev), None if bias is None else bias.to(dev))
    return flat, ClusteredItemCatalogue.from_assignment(flat, c["centroids"].to(dev), c["assign"].to(dev)).with_deep()


def _deep(dev):
    if "deep" not in _CACHE:
        c = deep_case()
        tags, bias = user_tags(c["assign"], 5), exact_bias(c["ids"].numel(), 7)
        s = (c["q"].to(torch.bfloat16).double() @ c["emb"].double().T).numpy()  # flat order, no prior
        _CACHE["deep"] = dict(c=c, tags=tags, bias=bias, s=s, q=c["q"].to(dev), filt=shape_filters(DEEP_Q, 6),
                              w=shape_weights(DEEP_Q), nb=_catalogues(c, tags, None, dev), b=_catalogues(c, tags, bias, dev))
    return _CACHE["deep"]


def _oracle_a(flat, L, probes, q, k, filt, ex, w, cur):
    f = restrict_to_probes(filt, probes.cpu(), L).to(q.device)
    ids, scores, _, _ = flat.topk(q, k, normalize_q=False, tag_filter=f, exclude_ids=ex, bias_weight=w,
                                  after_scores=None if cur is None else cur[0], after_ids=None if cur is None else cur[1])
    return scores, ids


def _oracle_b(cl, probes, q, k, filt, ex, w, cur, prior=True):
    cpu = lambda t: None if t is None else t.cpu()
    _, sc, ids = ivf_filt_checker(q.cpu().to(torch.bfloat16), cl.emb.cpu(), cl.row_ids.cpu(), cl.list_off.cpu(), probes.cpu(),
                                  k, None if ex is None else cl.rows_of(ex).cpu(), cpu(cl.tags), cpu(filt),
                                  cpu(cl.bias) if prior else None, cpu(w), None if cur is None else cur[0].cpu(),
                                  None if cur is None else cur[1].cpu())
    return torch.from_numpy(sc), torch.from_numpy(ids)


def _check(view, flat, q, k, nprobe, what, filt=None, ex=None, w=None, cur=None):
    probes = view.probe(q, nprobe, normalize_q=False)
    got = view.topk(q, k, nprobe=nprobe, normalize_q=False, exclude_ids=ex, tag_filter=filt, bias_weight=w,
                    after_scores=None if cur is None else cur[0], after_ids=None if cur is None else cur[1])
    assert got[0].dtype == torch.float32 and got[1].dtype == torch.int64 and got[0].shape == (q.shape[0], k)
    _same(got, _oracle_a(flat, view.nlist, probes, q, k, filt, ex, w, cur), ("A",) + what)
    _same(got, _oracle_b(view, probes, q, k, filt, ex, w, cur), ("B",) + what)
    return got


VARIANTS = {"none": ("", 0), "tags": ("t", 0), "prior": ("b", 0), "cursor": ("c", 0), "all": ("tbc", 0),
            "all_x1": ("tbc", 1), "all_x1024": ("tbc", 1024)}


def _cursors(S, parts):
    s = S["s"] + (S["w"].double().numpy()[:, None] * S["bias"].double().numpy()[None, :] if "b" in parts else 0.0)
    return shape_cursors(s, S["c"]["ids"], DEEP_Q, 22)  # a seed whose "id + 1" is an id the catalogue does not hold


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("k", DEEP_KS)
@pytest.mark.parametrize("nprobe", [1, 3, 10])
def test_shapes_against_both_oracles(dev, nprobe, k, variant):
    """Lists of 0 / 1 / 63 / 64 / 130 / 1,030 / 1,985 / 2,048 / 2,049 / 4,096 rows, 70 queries (the long list,
    every query's first probe, is served by two pair tiles), every option set.  The cursors cover an id
    inside a tie run, ids the catalogue does not hold, the extreme ids and scores +inf, -inf and NaN."""
    S = _deep(dev)
    parts, X = VARIANTS[variant]
    flat, view = S["b"] if "b" in parts else S["nb"]
    filt = S["filt"].to(dev) if "t" in parts else None
    w = S["w"].to(dev) if "b" in parts else None
    cur = tuple(t.to(dev) for t in _cursors(S, parts)) if "c" in parts else None
    ex = deep_exclude(S["c"], X).to(dev) if X else None
    got = _check(view, flat, S["q"], k, nprobe, (variant, nprobe, k), filt, ex, w, cur)
    empty = lambda i: bool((got[1][i] == 0).all()) and bool(torch.isneginf(got[0][i]).all())
    if not parts:
        assert bool((got[1] != 0).all())  # the long list alone fills every k
        if nprobe == 1:  # the long list's last k rows, the best first
            want = S["c"]["ids"][S["c"]["assign"] == LONG].flip(0)[:k].to(dev)
            assert torch.equal(got[1], want[None, :].expand(DEEP_Q, -1))
            assert torch.equal(got[0][0].cpu(), torch.arange(4095, 4095 - k, -1).float())
    if "t" in parts:
        assert empty(1) and empty(9)  # the unsatisfiable filter
    if "c" in parts:
        assert empty(5) and empty(6)  # cursor scores -inf and NaN


def test_pages_of_129_add_up_to_the_deep_list(dev):
    """Pages of k = 129, each behind the last (score, id) of the one before, with the same nprobe: chained
    to exhaustion they are the k = 1,024 list, whether a query's list ends inside it or fills it."""
    S = _deep(dev)
    q, (flat, view) = S["q"], S["b"]
    filt = torch.tensor([[15, 0, 0]] * DEEP_Q, dtype=torch.int32, device=dev)  # about one item in 16: fewer than 1,024
    filt[::2] = 0  # and every other query unfiltered: the long list alone fills its 1,024
    w = S["w"].to(dev)
    for nprobe in (1, 3):
        kw = dict(nprobe=nprobe, normalize_q=False, tag_filter=filt, bias_weight=w)
        long_s, long_i = view.topk(q, 1024, **kw)
        pages_s, pages_i = [], []
        cs = ci = None
        for _ in range(9):  # 8 pages cover 1,024; the ninth lies behind it
            ps, pi = view.topk(q, 129, after_scores=cs, after_ids=ci, **kw)
            pages_s.append(ps)
            pages_i.append(pi)
            cs, ci = ps[:, -1].contiguous(), pi[:, -1].contiguous()
        cat_s, cat_i = torch.cat(pages_s, dim=1), torch.cat(pages_i, dim=1)
        _same((cat_s[:, :1024], cat_i[:, :1024]), (long_s, long_i), ("pages", nprobe))
        n = (long_i != 0).sum(dim=1)
        assert int(n.min()) < 1024 and int(n.max()) == 1024  # both kinds of query occur
        short = n < 1024
        assert bool((cat_i[short][:, 1024:] == 0).all()) and bool((pages_i[-1][short] == 0).all())


def test_cursor_id_of_a_list_the_query_does_not_probe(dev):
    """nprobe = 1, so only the long list is scanned.  The cursor score is a score of the long list and the
    cursor id an id of another list, so the id term decides the one row that ties, through a cursor row
    that comes from a search in a list that does not hold the id."""
    S = _deep(dev)
    c, q, (flat, view) = S["c"], S["q"], S["nb"]
    other = torch.nonzero(c["assign"] != LONG)[:, 0]
    i = torch.arange(DEEP_Q)
    cs = (4000.0 - 7 * i).float().to(dev)
    ci = c["ids"][other[(i * 131) % other.numel()]].to(dev)
    for k in (129, 1024):
        got = _check(view, flat, q, k, 1, ("unprobed", k), cur=(cs, ci))
        tie = got[0][:, 0] == cs
        assert bool(tie.any()) and not bool(tie.all())  # the row that ties is returned iff its id is above the cursor's
        assert bool((got[1][:, 0][tie] > ci[tie]).all())


def _hand_case(dev):
    """Probe rows written by hand (pads, indices that are no list, the long list named twice, a short list
    named twice, pads only) with every feature at once, for the raw call and the script op."""
    S = _deep(dev)
    _, cl = S["b"]
    q = S["q"][:9]
    probes = torch.tensor([[9, -1, -1, -1], [-1, 5, -1, 7], [-1, -1, -1, -1], [11, 1000, -7, 6], [0, -1, -1, -1],
                           [8, 6, 9, 5], [-1, -1, -1, 4], [9, 9, -1, -1], [3, 3, 1, -1]], dtype=torch.int32, device=dev)
    s = S["s"][:9] + S["w"][:9].double().numpy()[:, None] * S["bias"].double().numpy()[None, :]
    cs, ci = shape_cursors(s, S["c"]["ids"], 9, 22)
    ex = deep_exclude(S["c"], 1)[:9].to(dev)
    return cl, q, probes, S["filt"][:9].contiguous().to(dev), S["w"][:9].contiguous().to(dev), cs.to(dev), ci.to(dev), ex


def test_probe_rows_with_pads_and_a_list_named_twice(dev):
    from recommendations_amd import kernels as K
    cl, q, probes, filt, w, cs, ci, ex = _hand_case(dev)
    xr = cl.rows_of(ex).contiguous()
    full = dict(exclude_rows=xr, tags=cl.tags, tag_filter=filt, bias=cl.bias, bias_weight=w, after_scores=cs, after_ids=ci)
    for names in ((), ("tags", "tag_filter"), ("bias", "bias_weight"), ("after_scores", "after_ids"), tuple(full)):
        kw = {n: full[n] for n in names}
        for k in (129, 1024):
            got = K.retrieve_ivf_topk(q, cl.emb, cl.row_ids, cl.list_off, probes, k, normalize_q=False, deep=True, **kw)
            want = _oracle_b(cl, probes, q, k, kw.get("tag_filter"), ex if "exclude_rows" in kw else None,
                             kw.get("bias_weight"), (cs, ci) if "after_ids" in kw else None, prior="bias" in kw)
            _same(got, want, (names, k))
            assert bool((got[1][2] == 0).all()) and bool((got[1][4] == 0).all())  # pads only; the empty list
    got = K.retrieve_ivf_topk(q, cl.emb, cl.row_ids, cl.list_off, probes, 1024, normalize_q=False, deep=True)
    assert torch.equal(got[1][7, 0::2], got[1][7, 1::2]) and torch.equal(bits(got[0][7, 0::2]), bits(got[0][7, 1::2]))
    assert int((got[1][8] != 0).sum()) == 2 * 64 + 1  # list 3 twice and the one-row list
    with pytest.raises(RuntimeError, match=r"retrieve_ivf_topk takes k in 1\.\.128 \(got 129\)"):
        K.retrieve_ivf_topk(q, cl.emb, cl.row_ids, cl.list_off, probes, 129)
    with pytest.raises(RuntimeError, match=r"retrieve_ivf_topk with deep=True takes k in 1\.\.1024 \(got 1025\)"):
        K.retrieve_ivf_topk(q, cl.emb, cl.row_ids, cl.list_off, probes, 1025, deep=True)


def test_k_100_through_the_new_entry_is_the_existing_entry(dev):
    """lthm_retrieve_ivf_topk_deep with k = 100 against lthm_retrieve_ivf_topk_filt, every feature on: the
    same workspace size and the same bits; and deep=True at k <= 128 through the Python call."""
    from recommendations_amd import _lib
    from recommendations_amd import kernels as K
    from recommendations_amd._lib import dcode, ptr, stream
    cl, q, probes, filt, w, cs, ci, ex = _hand_case(dev)
    xr = cl.rows_of(ex).contiguous()
    Q, N, L, P, k = 9, len(cl), cl.nlist, 4, 100
    lib = _lib.load()
    need = lib.lthm_retrieve_ivf_deep_ws_bytes(Q, N, L, P, k, 1, 1)
    assert need == lib.lthm_retrieve_ivf_filt_ws_bytes(Q, N, L, P, k, 1, 1)
    x, t, b, c = (_lib.STRUCTS[n]() for n in ("lthm_retrieve_excl", "lthm_retrieve_tags", "lthm_retrieve_bias",
                                               "lthm_retrieve_ivf_cursor"))
    x.rows, x.X = ptr(xr), 1
    t.tags, t.filter = ptr(cl.tags), ptr(filt)
    b.bias, b.weight = ptr(cl.bias), ptr(w)
    c.after_score, c.after_id = ptr(cs), ptr(ci)
    out = []
    for name in ("lthm_retrieve_ivf_topk_filt", "lthm_retrieve_ivf_topk_deep"):
        sc = torch.empty((Q, k), dtype=torch.float32, device=dev)
        ids = torch.empty((Q, k), dtype=torch.int64, device=dev)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        _lib.call(name, ptr(cl.emb), N, ptr(cl.row_ids), ptr(cl.list_off), L, ptr(q), dcode(q), 0, Q, ptr(probes), P, k,
                  *[ctypes.addressof(o) for o in (x, t, b, c)], ptr(sc), ptr(ids), ptr(ws), need, stream())
        out.append((sc, ids))
    _same(out[1], out[0], "entries")
    kw = dict(normalize_q=False, exclude_rows=xr, tags=cl.tags, tag_filter=filt, bias=cl.bias, bias_weight=w, after_scores=cs,
              after_ids=ci)
    _same(K.retrieve_ivf_topk(q, cl.emb, cl.row_ids, cl.list_off, probes, k, deep=True, **kw), out[0], "deep=True, k = 100")
    _same(K.retrieve_ivf_topk(q, cl.emb, cl.row_ids, cl.list_off, probes, k, **kw), out[0], "k = 100")


def test_chunked_queries_change_no_bit(dev, monkeypatch):
    """The chunk constant patched down to the workspace of 64 queries: Q = 70 splits at 64, and the result
    is the unsplit call's, with every per-query argument sliced along."""
    from recommendations_amd import _lib
    from recommendations_amd import kernels as K
    S = _deep(dev)
    q, (_, view) = S["q"], S["b"]
    cur = tuple(t.to(dev) for t in _cursors(S, "b"))
    ex = deep_exclude(S["c"], 1024).to(dev)
    kw = dict(nprobe=3, normalize_q=False, exclude_ids=ex, tag_filter=S["filt"].to(dev), bias_weight=S["w"].to(dev),
              after_scores=cur[0], after_ids=cur[1])
    whole = view.topk(q, 200, **kw)
    size = lambda n: _lib.load().lthm_retrieve_ivf_deep_ws_bytes(n, len(view), view.nlist, 3, 200, 1024, 1)
    assert size(DEEP_Q) < K.RETRIEVE_IVF_DEEP_WS_BYTES and size(64) < size(65)
    calls = []
    real = K.call
    monkeypatch.setattr(K, "call", lambda name, *a, **k: (calls.append((name, a[8] if name.endswith("ivf_topk_deep") else None)), real(name, *a, **k))[1])
    monkeypatch.setattr(K, "RETRIEVE_IVF_DEEP_WS_BYTES", size(64))
    _same(view.topk(q, 200, **kw), whole, "split at 64")
    assert [c for c in calls if c[0] == "lthm_retrieve_ivf_topk_deep"] == [("lthm_retrieve_ivf_topk_deep", 64),
                                                                          ("lthm_retrieve_ivf_topk_deep", 6)]
    monkeypatch.setattr(K, "RETRIEVE_IVF_DEEP_WS_BYTES", 1)  # never below one query per call
    first = {n: (v[:3] if isinstance(v, torch.Tensor) else v) for n, v in kw.items()}
    _same(view.topk(q[:3], 200, **first), tuple(t[:3] for t in whole), "one query per call")
    assert [c[1] for c in calls if c[0] == "lthm_retrieve_ivf_topk_deep"][2:] == [1, 1, 1]


def test_unit_vectors_every_list_equals_flat(dev):
    """N = 20,000 unit vectors in 64 lists, random tags, random finite bias, per-query weights: with every
    list probed the k = 1,024 list is to_flat().topk's, bit for bit, and so is recall's view of it."""
    from recommendations_amd.models.lthm.sequence.retrieval import ClusteredItemCatalogue, ItemCatalogue
    N, L, Q = 20000, 64, 64
    c = unit_case(N, L, Q, 41)
    g = torch.Generator().manual_seed(43)
    tags = torch.randint(0, 64, (N,), generator=g).to(torch.int32)
    bias = (0.1 * torch.randn(N, generator=g)).contiguous()
    flat = ItemCatalogue(c["ids"].to(dev), c["emb"].to(dev), tags.to(dev), bias.to(dev))
    filt = torch.stack([1 << torch.randint(0, 3, (Q,), generator=g), torch.zeros(Q, dtype=torch.int64),
                        8 << torch.randint(0, 3, (Q,), generator=g)], dim=1).to(torch.int32).to(dev)
    w = (2 * torch.rand(Q, generator=g)).to(dev)
    view = ClusteredItemCatalogue.from_assignment(flat, c["centroids"].to(dev), c["assign"].to(dev)).with_deep()
    q = c["q"].to(dev)
    for kw in (dict(), dict(tag_filter=filt, bias_weight=w)):
        got = view.topk(q, 1024, nprobe=64, **kw)
        ids, scores, _, _ = view.to_flat().topk(q, 1024, **kw)
        _same(got, (scores, ids), tuple(kw))
        assert bool((ids[:, -1] != 0).all())
    assert view.recall(q, 1024, 64, **kw) == 1.0 and 0.0 < view.recall(q, 1024, 2, **kw) < 1.0


def _diversify_case(dev):
    from recommendations_amd.models.lthm.sequence.retrieval import ClusteredItemCatalogue, ItemCatalogue
    emb, groups = exact_items()
    N = emb.shape[0]
    ids = spread_ids(N, 17)
    g = torch.Generator().manual_seed(19)
    assign = torch.randint(0, 7, (N,), generator=g)
    cen = torch.randint(-1, 2, (7, D), generator=g).to(torch.bfloat16)
    flat = ItemCatalogue(ids.to(dev), emb.to(dev), groups=groups.to(dev))
    view = ClusteredItemCatalogue.from_assignment(flat, cen.to(dev), assign.to(dev)).with_deep(groups.to(dev))
    return flat, view, emb, groups, ids


@pytest.mark.parametrize("cap", [None, 1, 2])
def test_diversify_equals_the_flat_catalogue_and_the_model(dev, cap):
    """A pool of 1,024 over exact items whose dots and scores tie in runs, k = 100: the view's diversify
    against ItemCatalogue.diversify on the same pool, all three outputs bit for bit (ties go to the lower
    id in both, though the clustered rows do not ascend with the ids), and against the fp64 greedy."""
    flat, view, emb, groups, ids = _diversify_case(dev)
    rows, scores, lam = exact_pool(1024)
    N = emb.shape[0]
    pool_ids = torch.where((rows >= 0) & (rows < N), ids[rows.clamp(0, N - 1).long()], torch.where(rows < 0, 0, 987654321098))
    pool_ids, scores, lam = pool_ids.to(dev), scores.to(dev), lam.to(dev)
    got = view.diversify(pool_ids, scores, 100, lam=lam, group_cap=cap)
    want = flat.diversify(pool_ids, scores, 100, lam=lam, group_cap=cap)
    for a, b, name in zip(got, want, ("item_ids", "scores", "objective")):
        assert a.dtype == b.dtype and a.shape == b.shape == (5, 100), name
        assert torch.equal(a.view(torch.int64) if a.dtype == torch.int64 else bits(a),
                           b.view(torch.int64) if b.dtype == torch.int64 else bits(b)), (name, cap)
    m_rows, m_scores, m_obj = greedy(rows, scores.cpu(), emb, 100, lam.cpu(), groups if cap is not None else None, cap or 1)
    m_ids = torch.where(torch.from_numpy(m_rows) >= 0, ids[torch.from_numpy(m_rows).clamp(min=0).long()], 0)
    assert torch.equal(got[0].cpu(), m_ids)
    assert torch.equal(bits(got[1].cpu()), bits(torch.from_numpy(m_scores)))
    assert torch.equal(bits(got[2].cpu() + 0.0), bits(torch.from_numpy(m_obj) + 0.0))
    assert bool((got[0][3] == 0).all())  # the query without a candidate
    # a number as lambda, and a pool that came from the view's own deep scan
    q = torch.randint(-2, 3, (5, D), generator=torch.Generator().manual_seed(23)).float().to(dev)
    sc, pid = view.topk(q, 1024, nprobe=3, normalize_q=False)
    for a, b in zip(view.diversify(pid, sc, 100, lam=0.5, group_cap=cap), flat.diversify(pid, sc, 100, lam=0.5, group_cap=cap)):
        assert torch.equal(a.view(torch.int64) if a.dtype == torch.int64 else bits(a),
                           b.view(torch.int64) if b.dtype == torch.int64 else bits(b)), cap


def test_script_op_equals_kernel_call(dev):
    from recommendations_amd import _lib
    from recommendations_amd import kernels as K
    _lib.load_torch_ops()
    cl, q, probes, filt, w, cs, ci, ex = _hand_case(dev)
    xr = cl.rows_of(ex).contiguous()
    op = torch.ops.lthm.retrieve_ivf_topk_deep

    @torch.jit.script
    def scripted(q, items, row_ids, list_off, probes, k: int, tags, filt, bias, w):
        return torch.ops.lthm.retrieve_ivf_topk_deep(q, items, row_ids, list_off, probes, k, False, None, tags, filt, bias, w)

    for k in (100, 300, 1024):
        for x, t, b, c in ((None, False, False, False), (xr, True, True, True), (None, True, False, False),
                           (xr, False, False, True)):
            want = K.retrieve_ivf_topk(q, cl.emb, cl.row_ids, cl.list_off, probes, k, normalize_q=False, exclude_rows=x,
                                       tags=cl.tags if t else None, tag_filter=filt if t else None, bias=cl.bias if b else None,
                                       bias_weight=w if b else None, after_scores=cs if c else None,
                                       after_ids=ci if c else None, deep=True)
            got = op(q, cl.emb, cl.row_ids, cl.list_off, probes, k, False, x, cl.tags if t else None, filt if t else None,
                     cl.bias if b else None, w if b else None, cs if c else None, ci if c else None)
            _same(got, want, (k, x is None, t, b, c))
        want = K.retrieve_ivf_topk(q, cl.emb, cl.row_ids, cl.list_off, probes, k, normalize_q=False, tags=cl.tags, tag_filter=filt,
                                   bias=cl.bias, bias_weight=w, deep=True)
        _same(scripted(q, cl.emb, cl.row_ids, cl.list_off, probes, k, cl.tags, filt, cl.bias, w), want, ("scripted", k))
    with pytest.raises(RuntimeError, match=r"retrieve_ivf_topk_deep takes k in 1\.\.1024, got 1025"):
        op(q, cl.emb, cl.row_ids, cl.list_off, probes, 1025, False)
    with pytest.raises(RuntimeError, match=r"k must be in 1\.\.128, got 129"):
        torch.ops.lthm.retrieve_ivf_topk_filt(q, cl.emb, cl.row_ids, cl.list_off, probes, 129, False)


def test_wrapper_retrieve_on_a_deep_view(dev):
    """LTHMModelWrapper.retrieve on a with_deep() view: k = 300 is the view's own deep list for the
    wrapper's query (and, with every list probed, the flat catalogue's); k = 20 with diversity and
    group_cap is the default pool of 160 from the deep scan, then the view's diversify."""
    from recommendations_amd.data import synthetic_lthm_batch
    from recommendations_amd.models.lthm.config import lthm_config
    from recommendations_amd.models.lthm.sequence.retrieval import ItemCatalogue, build_catalogue
    from recommendations_amd.models.lthm.sequence.wrapper import LTHMModelWrapper
    torch.manual_seed(0)
    cfg = lthm_config(T=30, d=64, n_layers=1, n_head=2, item_vocab=1000, lookahead=[0, 2, 4], out_emb_dim=D,
                      gradient_checkpointing=False)
    m = LTHMModelWrapper(cfg).to(dev).eval()
    batch = synthetic_lthm_batch(20, 30, seed=3, device=dev)
    ids = batch["product_ids"].reshape(-1)
    extra = torch.randint(1, 2 ** 62, (600,), generator=torch.Generator().manual_seed(5)).to(dev)
    built = build_catalogue(m, torch.cat([extra, ids[ids != 0]]), chunk=128)
    g = torch.Generator().manual_seed(9)
    N = len(built)
    groups = torch.randint(0, 5, (N,), generator=g).to(torch.int32).to(dev)
    flat = ItemCatalogue(built.ids, built.emb, torch.randint(0, 8, (N,), generator=g).to(torch.int32).to(dev),
                         (0.05 * torch.randn(N, generator=g)).to(dev), groups)
    plain = flat.cluster(8, iters=2)
    view = plain.with_deep(groups)
    out = m.forward(batch)
    q = out["next_token_emb"][:, -1, 0].contiguous()
    q = q if q.dtype in (torch.float32, torch.bfloat16) else q.float()
    for kw in (dict(), dict(tag_any=5, bias_weight=0.5, exclude_history=True)):
        got = m.retrieve(batch, view, 300, nprobe=3, **kw)
        assert sorted(got) == ["item_ids", "scores"] and got["item_ids"].shape == (20, 300)
        from recommendations_amd.models.lthm.sequence.retrieval import make_tag_filter
        hand = view.topk(q, 300, nprobe=3, exclude_ids=out["current_token_ids"] if kw else None,
                         tag_filter=make_tag_filter(20, 0, 5, 0, device=dev) if kw else None,
                         bias_weight=0.5 if kw else None)
        _same((got["scores"], got["item_ids"]), hand, kw)
        want = m.retrieve(batch, flat, 300, **kw)
        full = m.retrieve(batch, view, 300, nprobe=8, **kw)
        _same((full["scores"], full["item_ids"]), (want["scores"], want["item_ids"]), ("every list", kw))
        page = m.retrieve(batch, view, 300, nprobe=8, after=full, **kw)
        want2 = m.retrieve(batch, flat, 300, after=want, **kw)
        _same((page["scores"], page["item_ids"]), (want2["scores"], want2["item_ids"]), ("page 2", kw))
    got = m.retrieve(batch, view, 20, nprobe=3, diversity=0.5, group_cap=2)
    assert sorted(got) == ["item_ids", "objective", "scores"] and got["item_ids"].shape == (20, 20)
    pool_s, pool_i = view.topk(q, 160, nprobe=3)
    hand = view.diversify(pool_i, pool_s, 20, lam=0.5, group_cap=2)
    for name, h in zip(("item_ids", "scores", "objective"), hand):
        assert torch.equal(got[name].view(torch.int64) if h.dtype == torch.int64 else bits(got[name]),
                           h.view(torch.int64) if h.dtype == torch.int64 else bits(h)), name
    key = groups[flat.rows_of(got["item_ids"]).clamp(min=0).long()]
    for gk in range(1, 5):
        assert int(((key == gk) & (got["item_ids"] != 0)).sum(dim=1).max()) <= 2
    # with every list probed the diversified list is the flat catalogue's
    want = m.retrieve(batch, flat, 20, diversity=0.5, group_cap=2, pool=1024)
    got = m.retrieve(batch, view, 20, nprobe=8, diversity=0.5, group_cap=2, pool=1024)
    for name in ("item_ids", "scores", "objective"):
        assert torch.equal(got[name].view(torch.int64) if got[name].dtype == torch.int64 else bits(got[name]),
                           want[name].view(torch.int64) if want[name].dtype == torch.int64 else bits(want[name])), name
    with pytest.raises(ValueError, match="does not take heads"):
        m.retrieve(batch, view, 300, nprobe=3, heads=[0, 1])
    with pytest.raises(ValueError, match=r"takes k in 1\.\.128 \(got 300\)"):
        m.retrieve(batch, plain.with_filters(), 300, nprobe=3)
