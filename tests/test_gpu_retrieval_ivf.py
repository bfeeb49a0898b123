"""Clustered catalogues on the GPU (csrc/retrieve.hip retr_ivf_topk_k, lthm_retrieve_ivf_topk,
K.retrieve_ivf_topk, ClusteredItemCatalogue, LTHMModelWrapper.retrieve(nprobe=)).

The contract: per query the k first, under (score descending, id ascending), of the items of the
probed lists that are not excluded, every score the bits the flat scan returns.  Exact cases
(integer operands, tests/retrieval_ivf_case.py) are compared bit for bit against two oracles:
  A  the flat ItemCatalogue with the tag word 1 << list and a per-query tag_any over the probed
     lists (existing, tested code), with the same exclude_ids;
  B  the fp64 checker of retrieval_ivf_case.py.
The unit-vector case goes past the 32 tag bits (L = 200) and is held to the eps = 1e-5 rules of
tests/test_gpu_retrieval.py: f32 accumulation of 128 products of unit vectors errs by at most
128 * 2^-24 * sum|a_i b_i| <= 7.7e-6.
"""
import numpy as np
import pytest
import torch

from retrieval_ivf_case import BIG, D, SHAPE_Q, ivf_checker, prune_case, shapes_case, shapes_exclude, unit_case

pytestmark = pytest.mark.gpu

EPS = 1e-5
_CACHE = {}


def bits(t):
    return t.contiguous().view(torch.int32)


def _built(name, make, dev):
    """(case, flat ItemCatalogue with tags, ClusteredItemCatalogue) on the device, built once."""
    if name not in _CACHE:
        from recommendations_amd.models.lthm.sequence.retrieval import ClusteredItemCatalogue, ItemCatalogue
        c = make()
        flat = ItemCatalogue(c["ids"].to(dev), c["emb"].to(dev), None if "tags" not in c else c["tags"].to(dev))
        cl = ClusteredItemCatalogue.from_assignment(flat, c["centroids"].to(dev), c["assign"].to(dev))
        _CACHE[name] = (c, flat, cl)
    return _CACHE[name]


def _oracle_a(flat, probes, q, k, exclude_ids=None):
    """The flat scan restricted to the probed lists by tags: (scores, ids)."""
    from recommendations_amd.models.lthm.sequence.retrieval import make_tag_filter
    any_mask = (1 << probes.long().clamp(min=0)).masked_fill(probes < 0, 0).sum(dim=1)  # distinct lists: the sum is the OR
    filt = make_tag_filter(q.shape[0], tag_any=any_mask, device=q.device)
    ids, scores, _, _ = flat.topk(q, k, normalize_q=False, tag_filter=filt, exclude_ids=exclude_ids)
    return scores, ids


def _oracle_b(cl, probes, q, k, exclude_ids=None):
    xr = None if exclude_ids is None else cl.rows_of(exclude_ids).cpu()
    _, sc, ids, _ = ivf_checker(q.cpu().to(torch.bfloat16), cl.emb.cpu(), cl.row_ids.cpu(), cl.list_off.cpu(),
                                probes.cpu(), k, xr)
    return torch.from_numpy(sc), torch.from_numpy(ids)


def _same(got, want, what):
    assert torch.equal(got[1].cpu(), want[1].cpu()), what
    assert torch.equal(bits(got[0].cpu()), bits(want[0].cpu())), what


@pytest.mark.parametrize("k", [1, 10, 128])
@pytest.mark.parametrize("nprobe", [1, 3, 5])
def test_shapes_against_both_oracles(dev, nprobe, k):
    c, flat, cl = _built("shapes", shapes_case, dev)
    q = c["q"].to(dev)
    probes = cl.probe(q, nprobe, normalize_q=False)
    assert probes.shape == (SHAPE_Q, nprobe) and bool((probes[:, 0] == BIG).all())  # 70 pairs on one list: two tiles
    got = cl.topk(q, k, nprobe=nprobe, normalize_q=False)
    assert got[0].dtype == torch.float32 and got[1].dtype == torch.int64 and got[0].shape == (SHAPE_Q, k)
    _same(got, _oracle_a(flat, probes, q, k), ("A", nprobe, k))
    _same(got, _oracle_b(cl, probes, q, k), ("B", nprobe, k))


@pytest.mark.parametrize("k", [10, 128])
def test_full_probe_equals_flat(dev, k):
    c, flat, cl = _built("shapes", shapes_case, dev)
    q = c["q"].to(dev)
    got = cl.topk(q, k, nprobe=cl.nlist, normalize_q=False)
    ids, scores, _, _ = cl.to_flat().topk(q, k, normalize_q=False)
    _same(got, (scores, ids), k)
    qn = torch.randn((33, D), generator=torch.Generator().manual_seed(8)).to(dev)  # the normalising path too
    got = cl.topk(qn, k, nprobe=cl.nlist)
    ids, scores, _, _ = cl.to_flat().topk(qn, k)
    _same(got, (scores, ids), (k, "normalised"))


@pytest.mark.parametrize("X", [1, 1024])
@pytest.mark.parametrize("nprobe,k", [(1, 10), (3, 128), (5, 10)])
def test_exclusion_against_flat_with_tags(dev, nprobe, k, X):
    c, flat, cl = _built("shapes", shapes_case, dev)
    q = c["q"].to(dev)
    ex = shapes_exclude(c, X).to(dev)
    probes = cl.probe(q, nprobe, normalize_q=False)
    got = cl.topk(q, k, nprobe=nprobe, normalize_q=False, exclude_ids=ex)
    _same(got, _oracle_a(flat, probes, q, k, ex), ("A", nprobe, k, X))
    _same(got, _oracle_b(cl, probes, q, k, ex), ("B", nprobe, k, X))
    if X == 1024:
        assert bool((got[1][1] == 0).all()) and bool(torch.isneginf(got[0][1]).all())  # query 1 excludes everything
        big = c["ids"][c["assign"] == BIG].to(dev)
        assert not bool(torch.isin(got[1][0], big).any())                            # query 0 a whole probed list


@pytest.mark.parametrize("k", [128, 100])
def test_prune_pressure(dev, k):
    c, flat, cl = _built("prune", prune_case, dev)
    q = c["q"].to(dev)
    probes = cl.probe(q, 4, normalize_q=False)
    got = cl.topk(q, k, nprobe=4, normalize_q=False)
    _same(got, _oracle_a(flat, probes, q, k), ("A", k))
    _same(got, _oracle_b(cl, probes, q, k), ("B", k))
    long_ids = c["ids"][c["assign"] == 1]
    assert int(got[1][1, 0]) == int(long_ids[-1]) and float(got[0][1, 0]) == 2 * 4095.0


def test_many_lists_eps_rules(dev):
    """L = 200 (past the tag bits), N = 20,000 unit vectors, Q = 130, nprobe = 64, k = 100."""
    N, L, Q, P, k = 20000, 200, 130, 64, 100
    c, flat, cl = _built("unit", lambda: unit_case(N, L, Q, 31), dev)
    q = c["q"].to(dev)
    probes = cl.probe(q, P)
    got_s, got_i = cl.topk(q, k, nprobe=P)
    s, _, _, allowed = ivf_checker(c["q"].to(torch.bfloat16), cl.emb.cpu(), cl.row_ids.cpu(), cl.list_off.cpu(),
                                   probes.cpu(), k)
    g_rows = cl.rows_of(got_i).cpu().numpy()
    g_s, g_i = got_s.cpu().numpy(), got_i.cpu().numpy()
    for i in range(Q):
        a = allowed[i]
        kk = min(k, a.size)
        kth = np.sort(s[i, a])[::-1][kk - 1]
        # condition on the checker's own scores, before the GPU's are looked at
        assert int((np.abs(s[i, a] - kth) <= EPS).sum()) <= 4, "too many probed rows within eps of the k-th score"
    for i in range(Q):
        a = allowed[i]
        kk = min(k, a.size)
        kth = np.sort(s[i, a])[::-1][kk - 1]
        r = g_rows[i, :kk]
        assert (r >= 0).all() and len(set(r.tolist())) == kk
        assert np.isin(r, a).all()                                    # every returned item lies in a probed list
        assert (g_i[i, kk:] == 0).all() and np.isneginf(g_s[i, kk:]).all()
        assert np.abs(g_s[i, :kk].astype(np.float64) - s[i, r]).max() <= EPS
        must = a[s[i, a] > kth + EPS]                                 # no probed item beats the k-th by more than eps
        assert set(must.tolist()) <= set(r.tolist())
        assert (s[i, r] >= kth - EPS).all()
        assert (np.diff(g_s[i, :kk]) <= 0).all()


def test_probe_rows_with_pads(dev):
    """Probe rows given by hand: -1 pads, indices that are no list, fewer valid entries than P, a row
    of pads only (an empty result) and a list named twice (both copies, as the merge has it)."""
    from recommendations_amd import kernels as K
    c, flat, cl = _built("shapes", shapes_case, dev)
    q = c["q"][:9].to(dev)
    probes = torch.tensor([[2, -1, -1, -1], [-1, 0, -1, 4], [-1, -1, -1, -1], [5, 1000, -7, 3], [1, -1, -1, -1],
                           [4, 3, 2, 0], [-1, -1, -1, 2], [2, 2, -1, -1], [0, 4, 1, -1]], dtype=torch.int32, device=dev)
    for k in (10, 128):
        got = K.retrieve_ivf_topk(q, cl.emb, cl.row_ids, cl.list_off, probes, k, normalize_q=False)
        _same(got, _oracle_b(cl, probes, q, k), k)
        assert bool((got[1][2] == 0).all()) and bool(torch.isneginf(got[0][2]).all())  # pads only
        assert bool((got[1][4] == 0).all())                                             # the empty list
        assert bool((got[1][7, 0::2] == got[1][7, 1::2]).all())                         # a list twice: every item twice
    ex = shapes_exclude(c, 1024)[:9].to(dev)
    got = K.retrieve_ivf_topk(q, cl.emb, cl.row_ids, cl.list_off, probes, 10, normalize_q=False,
                              exclude_rows=cl.rows_of(ex).contiguous())
    _same(got, _oracle_b(cl, probes, q, 10, ex), "excl")


def test_cluster_builds(dev):
    from recommendations_amd import kernels as K
    from recommendations_amd.models.lthm.sequence.retrieval import ItemCatalogue
    N, L = 3000, 16
    c = unit_case(N, 24, 70, 5)
    tags = (torch.arange(N) % 7).to(torch.int32)
    flat = ItemCatalogue(c["ids"].to(dev), c["emb"].to(dev), tags.to(dev))
    a, b = flat.cluster(L, iters=3), flat.cluster(L, iters=3)
    for name in ("row_ids", "list_off", "tags"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    for name in ("emb", "centroids"):
        assert torch.equal(getattr(a, name).view(torch.int16), getattr(b, name).view(torch.int16)), name
    assert a.centroids.shape == (L, D) and a.centroids.dtype == torch.bfloat16 and len(a) == N
    assert torch.equal(torch.sort(a.row_ids)[0], flat.ids)          # every id in exactly one list
    assert int(a.list_lengths().sum()) == N and int(a.list_off[-1]) == N
    lists = torch.repeat_interleave(torch.arange(L, device=dev), a.list_lengths())
    same_list = lists[1:] == lists[:-1]
    assert bool((a.row_ids[1:] > a.row_ids[:-1])[same_list].all())  # id-ascending inside a list
    best = K.retrieve_topk(a.emb, a.centroids, 1, normalize_q=False)[1][:, 0].long()
    assert torch.equal(best, lists)                                 # every item sits with its best stored centroid
    back = a.to_flat()
    assert torch.equal(back.ids, flat.ids) and torch.equal(back.tags, flat.tags)
    assert torch.equal(back.emb.view(torch.int16), flat.emb.view(torch.int16))
    q = c["q"].to(dev)
    rec = [a.recall(q, 20, n) for n in (1, 2, 4, 8, 16)]
    assert all(x <= y for x, y in zip(rec, rec[1:])), rec
    assert rec[-1] == 1.0 and 0.0 < rec[0], rec
    assert len(flat.cluster(L, iters=1, seed=3, sample=500)) == N   # a sampled build keeps every item


def test_save_load_and_device_round_trip(dev, tmp_path):
    from recommendations_amd.models.lthm.sequence.retrieval import ClusteredItemCatalogue
    c, flat, cl = _built("shapes", shapes_case, dev)
    path = str(tmp_path / "ivf.safetensors")
    cl.save(path)
    again = ClusteredItemCatalogue.load(path, device=dev)
    q = c["q"].to(dev)
    _same(again.topk(q, 10, nprobe=3, normalize_q=False), cl.topk(q, 10, nprobe=3, normalize_q=False), "load")
    there = cl.to("cpu").to(dev)
    _same(there.topk(q, 10, nprobe=3, normalize_q=False), cl.topk(q, 10, nprobe=3, normalize_q=False), "to")
    assert torch.equal(again.row_ids, cl.row_ids) and torch.equal(again.list_off, cl.list_off)


def test_script_op_equals_kernel_call(dev):
    from recommendations_amd import _lib
    from recommendations_amd import kernels as K
    _lib.load_torch_ops()
    c, flat, cl = _built("shapes", shapes_case, dev)
    q = c["q"].to(dev)
    probes = cl.probe(q, 3, normalize_q=False)
    xr = cl.rows_of(shapes_exclude(c, 1024).to(dev)).contiguous()
    for x in (None, xr):
        want = K.retrieve_ivf_topk(q, cl.emb, cl.row_ids, cl.list_off, probes, 10, normalize_q=False, exclude_rows=x)
        got = torch.ops.lthm.retrieve_ivf_topk(q, cl.emb, cl.row_ids, cl.list_off, probes, 10, False, x)
        _same(got, want, x is None)


def test_refusals_on_the_device(dev):
    from recommendations_amd import kernels as K
    c, flat, cl = _built("shapes", shapes_case, dev)
    q = c["q"].to(dev)
    probes = cl.probe(q, 2, normalize_q=False)
    with pytest.raises(RuntimeError, match=r"takes k in 1\.\.128 \(got 129\)"):
        K.retrieve_ivf_topk(q, cl.emb, cl.row_ids, cl.list_off, probes, 129)
    with pytest.raises(RuntimeError, match=r"1\.\.64 probes per query \(got P=65\)"):
        K.retrieve_ivf_topk(q, cl.emb, cl.row_ids, cl.list_off, torch.zeros((SHAPE_Q, 65), dtype=torch.int32, device=dev), 5)
    with pytest.raises(RuntimeError, match=r"probes must be int32 \[Q, P\]"):
        K.retrieve_ivf_topk(q, cl.emb, cl.row_ids, cl.list_off, probes.long(), 5)
    with pytest.raises(RuntimeError, match=r"row_ids must be int64 \[N\]"):
        K.retrieve_ivf_topk(q, cl.emb, cl.row_ids[:-1].contiguous(), cl.list_off, probes, 5)
    with pytest.raises(RuntimeError, match=r"list_off must be int64 \[L \+ 1\]"):
        K.retrieve_ivf_topk(q, cl.emb, cl.row_ids, cl.list_off.int(), probes, 5)


def test_wrapper_retrieve_full_probe_equals_flat(dev):
    """LTHMModelWrapper.retrieve on the smallest configuration of tests/test_gpu_wrapper_api.py (T = 30, d = 64,
    one layer, two heads, lookahead [0, 2, 4]; the product tower 128 wide, as retrieval takes it)."""
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
    flat = build_catalogue(m, torch.cat([extra, ids[ids != 0]]), chunk=128)
    cl = flat.cluster(8, iters=2)
    for kw in (dict(), dict(exclude_history=True)):
        want = m.retrieve(batch, flat, 20, **kw)
        got = m.retrieve(batch, cl, 20, nprobe=8, **kw)
        assert torch.equal(got["item_ids"], want["item_ids"]), kw
        assert torch.equal(bits(got["scores"]), bits(want["scores"])), kw
    few = m.retrieve(batch, cl, 20, nprobe=2, exclude_history=True)
    seen = batch["product_ids"]
    assert not bool((few["item_ids"][:, :, None] == seen[:, None, :]).logical_and(few["item_ids"][:, :, None] != 0).any())
    with pytest.raises(ValueError, match="does not take heads"):
        m.retrieve(batch, cl, 20, nprobe=2, heads=[0, 1])
