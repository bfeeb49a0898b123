"""CPU checks of the tag-filter retrieval's host layer: the new C ABI entry and struct, the
checker the GPU tests use (retrieval_tags_case.py) pinned against a brute-force loop, and
ItemCatalogue with tags (constructor, from_embeddings, save / load, the filter helpers, bit 31 and
2^32 - 1).  No kernel is launched."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from recommendations_amd import _lib
from recommendations_amd import kernels as K
from recommendations_amd.models.lthm.sequence import retrieval as R
from recommendations_amd.models.lthm.sequence.retrieval import ItemCatalogue
from retrieval_tags_case import bits32, eligible, tags_checker

B31 = 1 << 31
ALL32 = (1 << 32) - 1


def test_symbols_and_struct():
    lib = _lib.load()
    assert hasattr(lib, "lthm_retrieve_topk_tags")
    protos = _lib.parse_header()
    assert protos["lthm_retrieve_topk_tags"] == ("int", ["lthm_retrieve_desc*", "lthm_retrieve_excl*",
                                                         "lthm_retrieve_group*", "lthm_retrieve_tags*", "void*"])
    assert lib.lthm_abi_version() == 44  # additive: nothing existing changed layout or signature
    st = _lib.STRUCTS["lthm_retrieve_tags"]
    assert [f[0] for f in st._fields_] == ["tags", "filter"] and ctypes.sizeof(st) == 16
    assert ctypes.sizeof(_lib.STRUCTS["lthm_retrieve_desc"]) == 104
    for fn in (K.retrieve_topk, K.retrieve_topk_group):
        p = inspect.signature(fn).parameters
        assert p["tags"].default is None and p["tag_filter"].default is None
        assert p["tags"].kind is inspect.Parameter.KEYWORD_ONLY
    from recommendations_amd.models.lthm.sequence.wrapper import LTHMModelWrapper
    p = inspect.signature(LTHMModelWrapper.retrieve).parameters
    assert all(p[n].default is None for n in ("tag_all", "tag_any", "tag_none"))
    assert inspect.signature(LTHMModelWrapper.catalogue_metrics).parameters["same_tags_mask"].default is None
    assert inspect.signature(R.build_catalogue).parameters["tags"].default is None


def test_abi_refuses_half_a_tags_struct():
    """With t, both pointers must be non-null: refused on the host, before any launch."""
    lib = _lib.load()
    d = _lib.STRUCTS["lthm_retrieve_desc"]()
    buf = (ctypes.c_char * 4096)()
    base = (ctypes.addressof(buf) + 255) // 256 * 256
    d.items = d.q = d.scores = d.rows = d.workspace = base
    d.Q, d.N, d.k, d.q_dtype, d.normalize_q, d.slab_rows = 1, 1, 1, _lib.F32, 0, 0
    d.ws_bytes = 1 << 30
    t = _lib.STRUCTS["lthm_retrieve_tags"]()
    for tags, filt in ((0, 0), (base, 0), (0, base), (base + 2, base), (base, base + 1)):
        t.tags, t.filter = tags or None, filt or None
        assert lib.lthm_retrieve_topk_tags(ctypes.addressof(d), None, None, ctypes.addressof(t), None) != 0


def brute(q, items, k, tags, filt, excl, trow):
    """The definition as Python loops over Python ints and floats."""
    U, G, D = q.shape
    N = items.shape[0]
    qs, it = q.double().tolist(), items.double().tolist()
    out_rows, out_sc, ranks, tss = [], [], [], []
    for u in range(U):
        fa, fy, fn = (int(v) & ALL32 for v in filt[u])
        s, ok = [], []
        for j in range(N):
            s.append(max(sum(a * b for a, b in zip(qs[u][g], it[j])) for g in range(G)))
            tj = int(tags[j]) & ALL32
            e = (tj & fa) == fa and (fy == 0 or (tj & fy) != 0) and (tj & fn) == 0
            ok.append(e and j not in [int(x) for x in excl[u]])
        cand = sorted((j for j in range(N) if ok[j]), key=lambda j: (-s[j], j))[:k]
        out_rows.append(cand + [-1] * (k - len(cand)))
        out_sc.append([s[j] for j in cand] + [float("-inf")] * (k - len(cand)))
        t = int(trow[u])
        if 0 <= t < N:
            ranks.append(sum(1 for j in range(N) if j != t and ok[j] and s[j] > s[t]))
            tss.append(s[t])
        else:
            ranks.append(-1)
            tss.append(float("-inf"))
    return (np.array(out_sc, dtype=np.float32), np.array(out_rows, dtype=np.int32), np.array(ranks, dtype=np.int32),
            np.array(tss, dtype=np.float32))


def test_checker_against_brute_force():
    g = torch.Generator().manual_seed(3)
    U, G, N, k = 5, 3, 23, 6
    q = torch.randint(-2, 3, (U, G, 128), generator=g).to(torch.bfloat16)
    items = torch.randint(-2, 3, (N, 128), generator=g).to(torch.bfloat16)
    items[7] = items[3]  # a tie
    tags = torch.randint(0, 16, (N,), generator=g).numpy().astype(np.int64)
    tags[::4] |= B31
    tags = tags.astype(np.uint32).view(np.int32)  # bit 31 as the int32 sign
    filt = np.array([[0, 0, 0], [1, 0, 0], [B31, 6, 0], [0, 0, B31 | 1], [3, 0, 2]], dtype=np.int64)
    excl = np.array([[-1, 2], [3, 3], [N, 5], [0, 1], [-5, 40]])
    trow = np.array([3, -1, 4, N, 0])
    e = eligible(tags, filt)
    assert e[0].all() and not e[4].any() and 0 < e[1].sum() < N and 0 < e[2].sum() < N and 0 < e[3].sum() < N
    b_sc, b_rows, b_rank, b_ts = brute(q, items, k, tags, filt, excl, trow)
    s, masked, sc, rows, rank, ts = tags_checker(q, items, k, tags, filt, excl, trow)
    assert np.array_equal(rows, b_rows) and np.array_equal(sc.view(np.uint32), b_sc.view(np.uint32))
    assert np.array_equal(rank, b_rank) and np.array_equal(ts.view(np.uint32), b_ts.view(np.uint32))
    assert (rows[4] == -1).all() and rank[4] == 0  # unsatisfiable: empty list, rank 0 for a valid target
    # a 2-D q is a group of one; without tags the filter term drops out
    s2 = tags_checker(q[:, 0], items, k, None, None, excl, trow)
    b2 = brute(q[:, :1], items, k, np.zeros(N, dtype=np.int64), np.zeros((U, 3), dtype=np.int64), excl, trow)
    assert np.array_equal(s2[3], b2[1]) and np.array_equal(s2[4], b2[2])
    # values in 0..2^32-1 and their int32 patterns are the same bits
    assert np.array_equal(bits32(np.array([-1, -(1 << 31)])), np.array([ALL32, B31]))
    assert np.array_equal(eligible(bits32(tags), filt), e)


def _cat(n=6, tags=True):
    ids = torch.tensor([50, 20, 40, 10, 60, 30][:n], dtype=torch.int64)
    emb = torch.arange(n * 128, dtype=torch.float32).view(n, 128).to(torch.bfloat16)
    tg = torch.tensor([5, 2, -4, 1, -(1 << 31), 7][:n], dtype=torch.int32) if tags else None
    return ids, emb, tg


def test_catalogue_with_tags_constructor():
    ids, emb, tg = _cat()
    order = torch.argsort(ids)
    cat = ItemCatalogue(ids[order], emb[order], tg[order])
    assert cat.tags.dtype == torch.int32 and cat.tags.is_contiguous() and torch.equal(cat.tags, tg[order])
    assert ItemCatalogue(ids[order], emb[order]).tags is None
    for bad in (tg[order].long(), tg[order][:-1], tg[order].view(2, 3), tg[order].float()):
        with pytest.raises(ValueError):
            ItemCatalogue(ids[order], emb[order], bad)
    # from_embeddings permutes the tags with the rows
    cat2 = ItemCatalogue.from_embeddings(ids, emb, tg)
    assert torch.equal(cat2.ids, ids[order]) and torch.equal(cat2.emb, emb[order]) and torch.equal(cat2.tags, tg[order])
    for i, t in zip(ids.tolist(), tg.tolist()):
        assert int(cat2.tags[cat2.rows_of(torch.tensor([i]))[0]]) == t
    assert ItemCatalogue.from_embeddings(ids, emb).tags is None
    with pytest.raises(ValueError):
        ItemCatalogue.from_embeddings(ids, emb, tg[:-1])
    assert torch.equal(cat2.to("cpu").tags, cat2.tags)
    # a catalogue without tags cannot filter: refused before any kernel is looked for
    with pytest.raises(ValueError):
        ItemCatalogue.from_embeddings(ids, emb).topk(torch.zeros(1, 128), 1, tag_filter=torch.zeros((1, 3), dtype=torch.int32))
    with pytest.raises(ValueError):
        ItemCatalogue.from_embeddings(ids, emb).filter_like(ids[:2], 1)


def test_save_load_round_trip(tmp_path):
    ids, emb, tg = _cat()
    with_tags = ItemCatalogue.from_embeddings(ids, emb, tg)
    without = ItemCatalogue.from_embeddings(ids, emb)
    a, b = str(tmp_path / "a.safetensors"), str(tmp_path / "b.safetensors")
    with_tags.save(a)
    without.save(b)
    la, lb = ItemCatalogue.load(a), ItemCatalogue.load(b)
    assert torch.equal(la.ids, with_tags.ids) and torch.equal(la.emb, with_tags.emb) and torch.equal(la.tags, with_tags.tags)
    assert la.tags.dtype == torch.int32
    assert lb.tags is None and torch.equal(lb.ids, without.ids) and torch.equal(lb.emb, without.emb)
    from safetensors import safe_open
    for path, keys in ((a, {"ids", "emb", "tags"}), (b, {"ids", "emb"})):
        with safe_open(path, framework="pt") as f:
            assert set(f.keys()) == keys and f.metadata() == {"format": "lthm-item-catalogue-v1"}
    assert R.FORMAT == "lthm-item-catalogue-v1"


def test_make_tag_filter():
    f = R.make_tag_filter(3, 5, 0, 2)
    assert f.dtype == torch.int32 and f.shape == (3, 3) and f.is_contiguous()
    assert f.tolist() == [[5, 0, 2]] * 3
    assert R.make_tag_filter(2).tolist() == [[0, 0, 0]] * 2
    # bit 31 and 2^32 - 1 wrap to the int32 with the same bits
    f = R.make_tag_filter(1, B31, ALL32, B31 | 1)
    assert f.tolist() == [[-(1 << 31), -1, -(1 << 31) + 1]]
    assert np.array_equal(bits32(f.numpy()), np.array([[B31, ALL32, B31 | 1]]))
    # tensors, one value per query; an int32 tensor's bit pattern is kept
    f = R.make_tag_filter(3, torch.tensor([1, B31, ALL32]), torch.tensor([0, 4, 8], dtype=torch.int32),
                          torch.tensor([-1, -2, 0], dtype=torch.int32))
    assert f.tolist() == [[1, 0, -1], [-(1 << 31), 4, -2], [-1, 8, 0]]
    assert R.make_tag_filter(2, torch.tensor(3), 0, 0).tolist() == [[3, 0, 0]] * 2
    for bad in (dict(tag_all=1 << 32), dict(tag_any=-(1 << 31) - 1), dict(tag_none=1.5), dict(tag_all=True),
                dict(tag_all=torch.tensor([1, 2])), dict(tag_any=torch.tensor([1.0, 2.0, 3.0])),
                dict(tag_none=torch.tensor([1 << 32, 0, 0]))):
        with pytest.raises(ValueError):
            R.make_tag_filter(3, **bad)
    with pytest.raises(ValueError):
        R.make_tag_filter(0)


def test_filter_like():
    ids, emb, tg = _cat()
    cat = ItemCatalogue.from_embeddings(ids, emb, tg)
    for mask in (0b110, B31 | 1, ALL32, 0):
        targets = torch.tensor([10, 60, 40, 77, 50], dtype=torch.int64)  # 77 is no catalogue id
        f = cat.filter_like(targets, mask)
        assert f.dtype == torch.int32 and f.shape == (5, 3)
        e = eligible(cat.tags.numpy(), f.numpy())
        tb = bits32(cat.tags.numpy())
        for i, t in enumerate(targets.tolist()):
            if t == 77:
                assert f[i].tolist() == [0, 0, 0] and e[i].all()
                continue
            r = int(cat.rows_of(torch.tensor([t]))[0])
            assert f[i, 1] == 0 and e[i, r]  # the target passes its own filter
            want = (tb & mask) == (tb[r] & mask)  # the same value in the masked field
            assert np.array_equal(e[i], want), (mask, t)
    assert bits32(cat.filter_like(torch.tensor([60]), B31).numpy()).tolist() == [[B31, 0, 0]]  # id 60 carries bit 31
    assert bits32(cat.filter_like(torch.tensor([10]), B31).numpy()).tolist() == [[0, 0, B31]]
    with pytest.raises(ValueError):
        cat.filter_like(targets, 1 << 32)


def test_unique_tags_follow_the_ids():
    ids = torch.tensor([9, 3, 9, 5, 3, 7], dtype=torch.int64)
    tg = torch.tensor([1, -2, 1, 4, -2, B31 - 1], dtype=torch.int32)
    out = R.unique_tags(ids, tg)
    assert torch.unique(ids).tolist() == [3, 5, 7, 9] and out.tolist() == [-2, 4, B31 - 1, 1] and out.dtype == torch.int32
    bad = tg.clone()
    bad[2] = 3  # id 9 with two different words
    with pytest.raises(ValueError, match="9"):
        R.unique_tags(ids, bad)
