"""Deep lists on clustered catalogues without a GPU: the fp64 checker of the GPU tests against a
brute-force sort at k > 128, the ABI surface of lthm_retrieve_ivf_topk_deep, the with_deep() view (storage,
.to, save / load), every new refusal with its message, and that the plain catalogue and the
with_filters() view keep theirs."""
import ctypes
import inspect
import re

import numpy as np
import pytest
import torch

from retrieval_ivf_case import D, shapes_case
from retrieval_ivf_deep_case import (DEEP_LENGTHS, DEEP_Q, LONG, brute_force_filt, deep_case, deep_exclude, exact_bias,
                                     ivf_filt_checker, user_tags)


def _toy():
    """Three lists of 150, 0 and 90 rows with heavy ties (eight distinct rows), ids interleaved."""
    g = torch.Generator().manual_seed(8)
    base = torch.randint(-1, 2, (8, D), generator=g)
    emb = base[torch.randint(0, 8, (240,), generator=g)].to(torch.bfloat16)
    perm = torch.randperm(240, generator=g) + 1
    row_ids = torch.cat([torch.sort(perm[:150])[0], torch.sort(perm[150:])[0]]) * 3 - 400  # ascending inside each list
    list_off = torch.tensor([0, 150, 150, 240], dtype=torch.int64)
    q = torch.randint(-1, 2, (5, D), generator=g).to(torch.bfloat16)
    probes = torch.tensor([[0, 2, 1], [2, -1, -1], [-1, -1, -1], [0, 0, 2], [1, 7, 0]], dtype=torch.int32)
    tags = torch.randint(0, 8, (240,), generator=g).to(torch.int32)
    bias = exact_bias(240, 3)
    return q, emb, row_ids, list_off, probes, tags, bias


def test_checker_against_brute_force_beyond_128():
    q, emb, row_ids, list_off, probes, tags, bias = _toy()
    filt = torch.tensor([[1, 0, 0], [0, 6, 0], [0, 0, 0], [0, 0, 4], [0, 0, 0]], dtype=torch.int32)
    weight = torch.tensor([2.0, -1.0, 0.5, 0.0, 1.0])
    ex = torch.tensor([[3, 200], [-1, 1000], [0, 0], [1, -1], [149, 150]], dtype=torch.int32)
    for k in (129, 200, 1024):
        for kw in (dict(), dict(tags=tags, tag_filter=filt), dict(bias=bias, weight=weight),
                   dict(tags=tags, tag_filter=filt, bias=bias, weight=weight, exclude_rows=ex)):
            s, sc, ids = ivf_filt_checker(q, emb, row_ids, list_off, probes, k, **kw)
            want = brute_force_filt(q, emb, row_ids, list_off, probes, k, **kw)
            cur = dict(kw, after_scores=torch.tensor([float(np.float32(s[i, 7 * i])) for i in range(5)]),
                       after_ids=row_ids[[0, 7, 14, 21, 28]].clone())
            for kk, (gs, gi), ww in ((kw, (sc, ids), want),
                                     (cur, ivf_filt_checker(q, emb, row_ids, list_off, probes, k, **cur)[1:],
                                      brute_force_filt(q, emb, row_ids, list_off, probes, k, **cur))):
                for i, w in enumerate(ww):
                    n = len(w)
                    assert [int(x) for x in gi[i, :n]] == [c[1] for c in w], (k, i)
                    assert [float(x) for x in gs[i, :n]] == [-c[0] + 0.0 for c in w], (k, i)
                    assert (gi[i, n:] == 0).all() and np.isneginf(gs[i, n:]).all()
            assert len(want[2]) == 0 and len(want[1]) <= 90
        # a list named twice gives both copies: without filters query 3 holds list 0 twice and list 2 once
        _, sc, ids = ivf_filt_checker(q, emb, row_ids, list_off, probes, k)
        n = min(k, 390)
        assert int((ids[3] != 0).sum()) == n
        if k >= 390:
            u, cnt = np.unique(ids[3, :390], return_counts=True)
            assert u.size == 240 and sorted(set(cnt.tolist())) == [1, 2]


def test_case_builders_cover_what_they_claim():
    c = deep_case()
    N = sum(DEEP_LENGTHS)
    assert c["ids"].numel() == N == 11466 and bool((c["ids"][1:] > c["ids"][:-1]).all())
    assert torch.bincount(c["assign"], minlength=len(DEEP_LENGTHS)).tolist() == DEEP_LENGTHS
    q, emb = c["q"].to(torch.bfloat16).double(), c["emb"].double()
    s = q @ emb[c["assign"] == LONG].T
    assert torch.equal(s, torch.arange(4096).double()[None, :].expand(DEEP_Q, -1))  # ascending with the row
    assert float((q @ emb[c["assign"] != LONG].T).abs().max()) <= 448
    probes = torch.argsort(-(q @ c["centroids"].double().T), dim=1, stable=True)
    assert bool((probes[:, 0] == LONG).all()) and len(set(probes[:, 1].tolist())) > 1
    tags = user_tags(c["assign"], 5)
    assert bool(((tags >> 16) == (1 << c["assign"]).to(torch.int32)).all())
    ex = deep_exclude(c, 1024)
    assert ex.shape == (DEEP_Q, 1024) and set(ex[0].tolist()) == set(c["ids"][c["assign"] == LONG][-1024:].tolist())
    assert bool((ex == 0).any()) and bool((ex == 987654321098).any())


def test_abi_surface():
    from recommendations_amd import _lib
    from recommendations_amd import kernels as K
    protos = _lib.parse_header()
    assert protos["lthm_retrieve_ivf_topk_deep"] == protos["lthm_retrieve_ivf_topk_filt"]
    assert protos["lthm_retrieve_ivf_deep_ws_bytes"] == protos["lthm_retrieve_ivf_filt_ws_bytes"] == (
        "int64_t", ["int64_t", "int64_t", "int64_t", "int32_t", "int32_t", "int64_t", "int32_t"])
    lib = _lib.load()
    with open(_lib.HEADER) as f:
        assert int(re.search(r"#define\s+LTHM_ABI_VERSION\s+(\d+)", f.read()).group(1)) == 44
    assert lib.lthm_abi_version() == 44  # additive
    assert lib.lthm_retrieve_ivf_topk_deep.restype is ctypes.c_int
    assert lib.lthm_retrieve_ivf_deep_ws_bytes.restype is ctypes.c_int64
    assert list(lib.lthm_retrieve_ivf_topk_deep.argtypes) == list(lib.lthm_retrieve_ivf_topk_filt.argtypes)
    sig = inspect.signature(K.retrieve_ivf_topk)
    assert sig.parameters["deep"].default is False and sig.parameters["deep"].kind is inspect.Parameter.KEYWORD_ONLY
    assert K.RETRIEVE_IVF_DEEP_WS_BYTES == 1 << 30
    dws, fws, ws = lib.lthm_retrieve_ivf_deep_ws_bytes, lib.lthm_retrieve_ivf_filt_ws_bytes, lib.lthm_retrieve_ivf_ws_bytes
    for args in ((256, 2_000_000, 4096, 8), (70, 11466, 10, 3), (1, 1, 1, 1), (4096, 2_000_000, 4096, 32)):
        Q, N, L, P = args
        for X in (0, 7, 1024):
            for cur in (0, 1):
                last = 0
                for k in (1, 2, 100, 128, 129, 200, 512, 1023, 1024):
                    got = dws(Q, N, L, P, k, X, cur)
                    assert got >= last > -1, (args, X, cur, k)  # monotone in k
                    last = got
                    if k <= 128:
                        assert got == fws(Q, N, L, P, k, X, cur), (args, X, cur, k)  # the existing path's size
                    else:
                        # the lists and the merge's input at this k, and 2,048 eight-byte slots per pair
                        assert got >= Q * P * 2048 * 8 + 12 * P * Q * k, (args, X, cur, k)
                        assert fws(Q, N, L, P, k, X, cur) == -1 and ws(Q, N, L, P, k, X) == -1  # they keep refusing
    for bad in ((0, 10, 1, 1, 200, 0), (1, 0, 1, 1, 200, 0), (1, 10, 0, 1, 200, 0), (1, 10, 1, 0, 200, 0), (1, 10, 1, 65, 200, 0),
                (1, 10, 1, 1, 0, 0), (1, 10, 1, 1, 1025, 0), (1, 10, 1, 1, 200, 1025), (1, 1 << 31, 1, 1, 200, 0),
                (1 << 26, 10, 1, 64, 200, 0)):
        assert dws(*bad, 0) == -1 and dws(*bad, 1) == -1, bad
    # invalid arguments are refused before any launch, with the library's error code (no GPU here)
    base = 1 << 12
    invalid = 1  # hipErrorInvalidValue

    def st(name, a, b):
        o = _lib.STRUCTS[name]()
        setattr(o, o._fields_[0][0], a)
        setattr(o, o._fields_[1][0], b)
        return o

    def call(t=None, b=None, c=None, x=None, **kw):
        keep = [o for o in (x, t, b, c) if o is not None]  # alive over the call
        return lib.lthm_retrieve_ivf_topk_deep(
            kw.get("items", base), 10, kw.get("row_ids", base), kw.get("list_off", base), 2, kw.get("q", base), _lib.F32, 1, 4,
            kw.get("probes", base), kw.get("P", 2), kw.get("k", 200),
            *[ctypes.addressof(o) if o is not None else None for o in (x, t, b, c)], kw.get("out_scores", base),
            kw.get("out_ids", base), kw.get("ws", base), kw.get("need", 1 << 40), None), keep

    need = dws(4, 10, 2, 2, 200, 0, 0)
    for kw in (dict(k=0), dict(k=1025), dict(P=65), dict(items=None), dict(need=need - 1), dict(need=16),
               dict(k=100, need=fws(4, 10, 2, 2, 100, 0, 0) - 1),
               dict(items=base + 8), dict(q=base + 4), dict(ws=base + 8), dict(row_ids=base + 4), dict(list_off=base + 4),
               dict(probes=base + 2), dict(out_scores=base + 2), dict(out_ids=base + 4),
               dict(t=st("lthm_retrieve_tags", base + 2, base)), dict(b=st("lthm_retrieve_bias", base + 1, None)),
               dict(c=st("lthm_retrieve_ivf_cursor", base, base + 4)), dict(x=st("lthm_retrieve_excl", base + 2, 4)),
               # a workspace that holds the call without a cursor but not the cursor rows
               dict(c=st("lthm_retrieve_ivf_cursor", base, base), need=need)):
        assert call(**kw)[0] == invalid, kw


def _clustered(groups=False, **kw):
    from recommendations_amd.models.lthm.sequence.retrieval import ClusteredItemCatalogue, ItemCatalogue
    c = shapes_case()
    flat = ItemCatalogue(c["ids"], c["emb"], kw.get("tags"), kw.get("bias"))
    return flat, ClusteredItemCatalogue.from_assignment(flat, c["centroids"], c["assign"]), c


def test_view_shares_storage_and_round_trips(tmp_path):
    from recommendations_amd.models.lthm.sequence.retrieval import (ClusteredItemCatalogue, DeepClusteredItemCatalogue,
                                                                    FilteredClusteredItemCatalogue)
    c = shapes_case()
    flat, cl, _ = _clustered(tags=user_tags(c["assign"], 5), bias=exact_bias(258, 7))
    groups = (torch.arange(258) % 7).to(torch.int32)  # in to_flat()'s order
    assert cl.scans_deep is False and cl.with_filters().scans_deep is False
    v = cl.with_deep(groups)
    assert v.scans_deep is True and v.scans_filters is True and cl.scans_deep is False and v is not cl
    assert isinstance(v, DeepClusteredItemCatalogue) and isinstance(v, FilteredClusteredItemCatalogue)
    assert v.with_deep() is v and v.with_filters() is v
    from_view = cl.with_filters().with_deep()
    assert type(from_view) is DeepClusteredItemCatalogue and from_view.groups is None and not from_view.has_groups
    for name in ("row_ids", "emb", "list_off", "centroids", "tags", "bias"):
        assert getattr(v, name).data_ptr() == getattr(cl, name).data_ptr(), name
        assert getattr(from_view, name).data_ptr() == getattr(cl, name).data_ptr(), name
    assert len(v) == len(cl) and v.nlist == cl.nlist and v.has_tags and v.has_bias and v.has_groups
    # the groups follow the items: clustered row r holds the item with id row_ids[r]
    assert torch.equal(v.groups, groups[flat.rows_of(cl.row_ids).long()]) and v.groups.dtype == torch.int32
    other = v.with_deep((torch.arange(258) % 3).to(torch.int32))
    assert other is not v and int(other.groups.max()) == 2 and int(v.groups.max()) == 6
    moved = v.to("cpu")
    assert moved.scans_deep is True and torch.equal(moved.groups, v.groups)  # .to keeps the flag and the groups
    assert cl.to("cpu").scans_deep is False and cl.with_filters().to("cpu").scans_deep is False
    p_view, p_plain = str(tmp_path / "view.safetensors"), str(tmp_path / "plain.safetensors")
    v.save(p_view)
    cl.save(p_plain)
    from safetensors import safe_open
    with safe_open(p_view, framework="pt") as a, safe_open(p_plain, framework="pt") as b:
        assert a.metadata() == b.metadata() and sorted(a.keys()) == sorted(b.keys())  # today's file: no flag, no groups
        for name in a.keys():
            x, y = a.get_tensor(name), b.get_tensor(name)
            assert x.dtype == y.dtype and torch.equal(x.view(torch.uint8), y.view(torch.uint8)), name
    again = ClusteredItemCatalogue.load(p_view)
    assert again.scans_deep is False and type(again) is ClusteredItemCatalogue
    assert list(inspect.signature(v.topk).parameters) == list(inspect.signature(cl.with_filters().topk).parameters)
    assert list(inspect.signature(v.diversify).parameters) == list(inspect.signature(flat.diversify).parameters)
    assert not hasattr(cl, "diversify") and not hasattr(cl.with_filters(), "diversify")


def test_view_refusals_with_their_messages():
    from recommendations_amd.models.lthm.sequence.wrapper import LTHMModelWrapper
    c = shapes_case()
    q = torch.zeros((2, D))
    _, cl, _ = _clustered(tags=user_tags(c["assign"], 5), bias=exact_bias(258, 7))
    for bad in (torch.zeros(258, dtype=torch.int64), torch.zeros(257, dtype=torch.int32), [0] * 258):
        with pytest.raises(ValueError, match=r"with_deep takes groups int32 \[N\], one key per item in to_flat\(\)'s order"):
            cl.with_deep(bad)
    v = cl.with_deep((torch.arange(258) % 7).to(torch.int32))
    bare = cl.with_deep()
    with pytest.raises(ValueError, match=r"a clustered catalogue takes k in 1\.\.1024 \(got 1025\)"):
        v.topk(q, 1025, nprobe=2)
    with pytest.raises(ValueError, match=r"a clustered catalogue takes k in 1\.\.1024 \(got 0\)"):
        v.topk(q, 0, nprobe=2)
    with pytest.raises(ValueError, match=r"nprobe takes at most the 5 lists there are \(got 6\)"):
        v.topk(q, 200, nprobe=6)
    with pytest.raises(ValueError, match=r"after_scores and after_ids are given together or neither"):
        v.topk(q, 200, nprobe=2, after_scores=torch.zeros(2))
    with pytest.raises(ValueError, match=r"tag_filter must be int32 \[Q, 3\]"):
        v.topk(q, 200, nprobe=2, tag_filter=torch.zeros((2, 2), dtype=torch.int32))
    with pytest.raises(RuntimeError, match="MI355X"):  # no CPU fall-back for the scan itself
        v.topk(q, 200, nprobe=2)
    ids, sc = torch.ones((2, 8), dtype=torch.int64), torch.zeros((2, 8))
    with pytest.raises(ValueError, match=r"diversify takes int64 item_ids \[Q, M\] \(got torch.int32"):
        v.diversify(ids.int(), sc, 4)
    with pytest.raises(ValueError, match=r"diversify takes f32 scores of the ids' shape"):
        v.diversify(ids, sc[:, :7], 4)
    with pytest.raises(ValueError, match=r"group_cap given, but this catalogue carries no groups"):
        bare.diversify(ids, sc, 4, group_cap=1)
    with pytest.raises(ValueError, match=r"diversify takes a pool of 1\.\.1024 candidates \(got M=1025\)"):
        v.diversify(torch.ones((2, 1025), dtype=torch.int64), torch.zeros((2, 1025)), 4)
    with pytest.raises(ValueError, match=r"diversify takes k in 1\.\.128 \(got 129\)"):
        v.diversify(ids, sc, 129)
    with pytest.raises(ValueError, match=r"group_cap takes an int >= 1 \(got 0\)"):
        v.diversify(ids, sc, 4, group_cap=0)
    with pytest.raises(ValueError, match=r"lam must lie in \[0, 1\] \(got 1.5\)"):
        v.diversify(ids, sc, 4, lam=1.5)
    with pytest.raises(ValueError, match=r"lam must be a number or a float tensor \[Q\]"):
        v.diversify(ids, sc, 4, lam=torch.zeros(3))
    # the wrapper on a deep view, before the forward
    retrieve = LTHMModelWrapper.retrieve
    for kw in (dict(heads=[0, 1]), dict(heads=[0], diversity=0.5)):
        with pytest.raises(ValueError, match=r"clustered catalogue does not take heads: use catalogue.to_flat\(\)"):
            retrieve(None, {}, v, 5, nprobe=2, **kw)
    with pytest.raises(ValueError, match=r"after given with diversity / group_cap: a cursor has no meaning"):
        retrieve(None, {}, v, 5, nprobe=2, diversity=0.5, after=(sc[:, 0], ids[:, 0]))
    with pytest.raises(ValueError, match=r"a clustered catalogue takes k in 1\.\.1024 \(got 1025\)"):
        retrieve(None, {}, v, 1025, nprobe=2)
    with pytest.raises(ValueError, match=r"a diversified list takes k in 1\.\.128 \(got 200\)"):
        retrieve(None, {}, v, 200, nprobe=2, diversity=0.5)
    with pytest.raises(ValueError, match=r"pool takes k\.\.1024 candidates \(got pool=2000, k=5\)"):
        retrieve(None, {}, v, 5, nprobe=2, diversity=0.5, pool=2000)
    with pytest.raises(ValueError, match=r"pool given without diversity or group_cap"):
        retrieve(None, {}, v, 5, nprobe=2, pool=64)
    with pytest.raises(ValueError, match=r"diversity takes lambda in \[0, 1\] \(got 2\)"):
        retrieve(None, {}, v, 5, nprobe=2, diversity=2)
    with pytest.raises(ValueError, match=r"group_cap given, but this catalogue carries no groups"):
        retrieve(None, {}, bare, 5, nprobe=2, group_cap=2)
    with pytest.raises(ValueError, match=r"takes nprobe, the lists each query scans"):
        retrieve(None, {}, v, 5, diversity=0.5)
    with pytest.raises(ValueError, match=r"pass catalogue.to_flat\(\)"):
        LTHMModelWrapper.catalogue_metrics(None, {}, v)


def test_plain_and_filtered_catalogues_are_what_they_were():
    from recommendations_amd import kernels as K
    from recommendations_amd.models.lthm.sequence.retrieval import ClusteredItemCatalogue, FilteredClusteredItemCatalogue
    from recommendations_amd.models.lthm.sequence.wrapper import LTHMModelWrapper
    c = shapes_case()
    _, cl, _ = _clustered(tags=user_tags(c["assign"], 5), bias=exact_bias(258, 7))
    view = cl.with_filters()
    assert type(cl) is ClusteredItemCatalogue and type(view) is FilteredClusteredItemCatalogue
    assert list(inspect.signature(cl.topk).parameters) == ["q", "k", "nprobe", "normalize_q", "exclude_ids"]
    assert list(inspect.signature(view.topk).parameters) == ["q", "k", "nprobe", "normalize_q", "exclude_ids", "tag_filter",
                                                             "after_scores", "after_ids", "bias_weight"]
    q = torch.zeros((2, D))
    retrieve = LTHMModelWrapper.retrieve
    for cat in (cl, view):
        with pytest.raises(ValueError, match=r"a clustered catalogue takes k in 1\.\.128 \(got 129\)"):
            cat.topk(q, 129, nprobe=2)
        with pytest.raises(ValueError, match=r"a clustered catalogue takes k in 1\.\.128 \(got 129\)"):
            retrieve(None, {}, cat, 129, nprobe=2)
        for kw, names in ((dict(diversity=0.5), "diversity"), (dict(pool=64), "pool"), (dict(group_cap=2), "group_cap"),
                          (dict(heads=[0, 1]), "heads")):
            with pytest.raises(ValueError, match=rf"clustered catalogue does not take {names}: use catalogue.to_flat\(\)"):
                retrieve(None, {}, cat, 5, nprobe=2, **kw)
    # the kernel call without deep keeps today's message; with it, the deep range
    t = torch.zeros(1)
    with pytest.raises(RuntimeError, match="MI355X"):
        K.retrieve_ivf_topk(t, t, t, t, t, 129)
