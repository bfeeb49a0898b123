"""CPU checks of the score prior's host layer: the new C ABI entry and struct, the refusals the
call makes before any launch, the checker the GPU tests use (retrieval_bias_case.py) pinned against
a brute-force loop with every composition, and ItemCatalogue's handling of a bias (save / load,
the permutation of from_embeddings and unique_bias, the refusals).  No kernel is launched."""
import ctypes
import inspect
import math
import struct

import numpy as np
import pytest
import torch

from recommendations_amd import _lib
from recommendations_amd import kernels as K
from recommendations_amd.models.lthm.sequence.retrieval import ItemCatalogue, unique_bias
from retrieval_bias_case import bias_checker, bias_scores

ALL32 = (1 << 32) - 1


def test_symbols_and_struct():
    lib = _lib.load()
    assert hasattr(lib, "lthm_retrieve_topk_bias")
    protos = _lib.parse_header()
    assert protos["lthm_retrieve_topk_bias"] == ("int", ["lthm_retrieve_desc*", "lthm_retrieve_excl*",
                                                         "lthm_retrieve_group*", "lthm_retrieve_tags*",
                                                         "lthm_retrieve_cursor*", "lthm_retrieve_bias*", "void*"])
    assert lib.lthm_abi_version() == 44  # additive: nothing existing changed layout or signature
    st = _lib.STRUCTS["lthm_retrieve_bias"]
    assert [f[0] for f in st._fields_] == ["bias", "weight"] and ctypes.sizeof(st) == 16
    assert ctypes.sizeof(_lib.STRUCTS["lthm_retrieve_desc"]) == 104
    assert ctypes.sizeof(_lib.STRUCTS["lthm_retrieve_cursor"]) == 16
    for fn in (K.retrieve_topk, K.retrieve_topk_group):
        p = inspect.signature(fn).parameters
        assert p["bias"].default is None and p["bias_weight"].default is None
        assert p["bias"].kind is inspect.Parameter.KEYWORD_ONLY
    assert inspect.signature(ItemCatalogue.topk).parameters["bias_weight"].default is None
    assert inspect.signature(ItemCatalogue.__init__).parameters["bias"].default is None
    from recommendations_amd.models.lthm.sequence.retrieval import build_catalogue
    from recommendations_amd.models.lthm.sequence.wrapper import LTHMModelWrapper
    assert inspect.signature(build_catalogue).parameters["bias"].default is None
    assert inspect.signature(LTHMModelWrapper.retrieve).parameters["bias_weight"].default is None
    assert inspect.signature(LTHMModelWrapper.catalogue_metrics).parameters["bias_weight"].default is None


def test_abi_refuses_a_bad_bias_struct():
    """With b, bias must be non-null and both pointers 4-byte aligned: refused on the host, before
    any launch."""
    lib = _lib.load()
    d = _lib.STRUCTS["lthm_retrieve_desc"]()
    buf = (ctypes.c_char * 4096)()
    base = (ctypes.addressof(buf) + 255) // 256 * 256
    d.items = d.q = d.scores = d.rows = d.workspace = base
    d.Q, d.N, d.k, d.q_dtype, d.normalize_q, d.slab_rows = 1, 1, 1, _lib.F32, 0, 0
    d.ws_bytes = 1 << 30
    b = _lib.STRUCTS["lthm_retrieve_bias"]()
    g = _lib.STRUCTS["lthm_retrieve_group"]()
    for G in (1, 3):
        g.G = G
        for bias, weight in ((0, 0), (0, base), (base + 2, 0), (base + 1, base), (base, base + 2), (base, base + 1)):
            b.bias, b.weight = bias or None, weight or None
            assert lib.lthm_retrieve_topk_bias(ctypes.addressof(d), None, ctypes.addressof(g), None, None,
                                               ctypes.addressof(b), None) != 0


def f32(x):
    return struct.unpack("f", struct.pack("f", x))[0]


def brute(q, items, k, bias, w, asc, arow, tags, filt, excl, trow):
    """The definition as Python loops over Python ints and floats.  Operands are small integers and
    the priors multiples of 0.5, so every float below is exact."""
    U, G, D = q.shape
    N = items.shape[0]
    qs, it = q.double().tolist(), items.double().tolist()
    out_rows, out_sc, ranks, tss = [], [], [], []
    for u in range(U):
        fa, fy, fn = (int(v) & ALL32 for v in filt[u])
        cs, cr = f32(float(asc[u])), int(arow[u])
        s, ok = [], []
        for j in range(N):
            dot = max(sum(a * b for a, b in zip(qs[u][g], it[j])) for g in range(G))
            sj = dot + float(w[u]) * float(bias[j])
            s.append(sj)
            tj = int(tags[j]) & ALL32
            e = (tj & fa) == fa and (fy == 0 or (tj & fy) != 0) and (tj & fn) == 0
            s32 = f32(sj)
            behind = (not math.isnan(cs)) and (s32 < cs or (s32 == cs and j > cr))
            ok.append(e and behind and j not in [int(x) for x in excl[u]])
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


@pytest.mark.parametrize("seed", range(12))
def test_checker_against_brute_force(seed):
    """A dozen random small cases; every one composes the prior with groups (G in 1..3), a tag
    filter, a cursor inside the biased order and an exclusion list that holds the target."""
    g = torch.Generator().manual_seed(100 + seed)
    U, G, N, k = 5, 1 + seed % 3, 23 + seed, 6 + seed % 4
    q = torch.randint(-1, 2, (U, G, 128), generator=g).to(torch.bfloat16)
    items = torch.randint(-1, 2, (N, 128), generator=g).to(torch.bfloat16)
    items[N // 2] = items[1]
    bias = (torch.randint(-8, 9, (N,), generator=g).float() * 0.5).numpy()
    w = np.array([0.0, 0.5, 1.0, 2.0, -1.0], dtype=np.float32)[(np.arange(U) + seed) % 5]
    plain = bias_checker(q, items, N, bias, w)
    # the cursor of user u: entry u + 1 of its own biased order (the last user: +inf, no cursor)
    asc = np.array([plain["scores"][u, u + 1] for u in range(U)], dtype=np.float32)
    arow = np.array([plain["rows"][u, u + 1] for u in range(U)], dtype=np.int64)
    asc[U - 1], arow[U - 1] = np.inf, -1
    tags = torch.randint(0, 4, (N,), generator=g).numpy().astype(np.int64)
    filt = np.zeros((U, 3), dtype=np.int64)
    filt[0] = [1, 0, 0]
    filt[1] = [0, 0, 2]
    filt[2] = [0, 3, 0]
    trow = np.array([3, N - 1, -1, N, 0])
    excl = np.full((U, 3), -1)
    excl[:, 0] = np.where(trow < N, trow, -1)  # the target inside its own list
    excl[:, 1] = torch.randint(0, N, (U,), generator=g).numpy()
    b_sc, b_rows, b_rank, b_ts = brute(q, items, k, bias, w, asc, arow, tags, filt, excl, trow)
    c = bias_checker(q, items, k, bias, w, asc, arow, tags, filt, excl, trow)
    assert np.array_equal(c["rows"], b_rows) and np.array_equal(c["scores"].view(np.uint32), b_sc.view(np.uint32))
    assert np.array_equal(c["rank"], b_rank) and np.array_equal(c["tscore"].view(np.uint32), b_ts.view(np.uint32))
    for u in range(U):  # eps = 0: near is the tie run of each rank, and it holds the row chosen
        for i, r in enumerate(c["rows"][u]):
            if r >= 0:
                assert r in c["near"][u][i]
                assert all(c["masked"][u, j] == c["s"][u, r] for j in c["near"][u][i])


def test_checker_neutral_cases_and_parts():
    g = torch.Generator().manual_seed(7)
    q = torch.randint(-1, 2, (4, 2, 128), generator=g).to(torch.bfloat16)
    items = torch.randint(-1, 2, (40, 128), generator=g).to(torch.bfloat16)
    bias = (torch.randint(-8, 9, (40,), generator=g).float() * 0.5).numpy()
    trow = np.array([0, 39, -1, 7])
    from retrieval_after_case import after_checker
    ref = after_checker(q, items, 9, trow=trow)
    for kw in (dict(bias=bias, w=np.zeros(4, dtype=np.float32)), dict(bias=np.zeros(40, dtype=np.float32)), dict()):
        c = bias_checker(q, items, 9, trow=trow, **kw)
        assert np.array_equal(c["rows"], ref[3]) and np.array_equal(c["scores"], ref[2])
        assert np.array_equal(c["rank"], ref[4]) and np.array_equal(c["tscore"], ref[5])
    # w None is 1; the prior is added after the maximum over the heads
    a, b = bias_scores(q, items, bias), bias_scores(q, items, bias, np.ones(4, dtype=np.float32))
    assert np.array_equal(a, b)
    heads = np.stack([bias_scores(q[:, h], items, bias) for h in range(2)])
    assert np.array_equal(a, heads.max(axis=0))
    # the prior makes and breaks ties: equal dots with different biases order by the bias
    it2 = items[:1].repeat(3, 1)
    c = bias_checker(q[:1, 0], it2, 3, np.array([0.0, 1.0, 0.5], dtype=np.float32))
    assert c["rows"][0].tolist() == [1, 2, 0]
    c = bias_checker(q[:1, 0], it2, 3, np.array([0.0, 1.0, 0.5], dtype=np.float32), np.array([-1.0], dtype=np.float32))
    assert c["rows"][0].tolist() == [0, 2, 1]


def _cat(n=6, bias=True, tags=False):
    ids = torch.arange(1, n + 1, dtype=torch.int64) * 10
    emb = torch.zeros((n, 128), dtype=torch.bfloat16)
    emb[:, 0] = torch.arange(n).to(torch.bfloat16)
    return ItemCatalogue(ids, emb, torch.arange(n, dtype=torch.int32) if tags else None,
                         torch.arange(n, dtype=torch.float32) * 0.25 - 0.5 if bias else None)


def test_catalogue_save_load_round_trip(tmp_path):
    for bias, tags in ((True, False), (True, True), (False, True), (False, False)):
        cat = _cat(bias=bias, tags=tags)
        path = str(tmp_path / f"cat_{int(bias)}{int(tags)}.safetensors")
        cat.save(path)
        back = ItemCatalogue.load(path)
        assert torch.equal(back.ids, cat.ids) and torch.equal(back.emb, cat.emb)
        assert (back.bias is None) == (not bias) and (back.tags is None) == (not tags)
        if bias:
            assert back.bias.dtype == torch.float32 and torch.equal(back.bias, cat.bias)
        assert (back.to("cpu").bias is None) == (not bias)
    # a file written before catalogues carried a bias: the two (or three) tensors only
    from safetensors.torch import save_file
    from recommendations_amd.models.lthm.sequence.retrieval import FORMAT
    cat = _cat(bias=False, tags=True)
    old = str(tmp_path / "old.safetensors")
    save_file({"ids": cat.ids, "emb": cat.emb, "tags": cat.tags}, old, metadata={"format": FORMAT})
    back = ItemCatalogue.load(old)
    assert back.bias is None and torch.equal(back.tags, cat.tags)


def test_bias_follows_the_permutation():
    g = torch.Generator().manual_seed(1)
    ids = torch.randperm(50, generator=g).to(torch.int64) + 1
    emb = torch.zeros((50, 128), dtype=torch.bfloat16)
    emb[:, 0] = ids.to(torch.bfloat16)
    bias = ids.float() * 0.5
    cat = ItemCatalogue.from_embeddings(ids, emb, bias=bias)
    assert torch.equal(cat.ids, torch.arange(1, 51)) and torch.equal(cat.bias, cat.ids.float() * 0.5)
    assert torch.equal(cat.emb[:, 0].float(), cat.ids.to(torch.bfloat16).float())
    # what build_catalogue does with the ids it is given: sorted, de-duplicated, one bias per id
    dup = torch.cat([ids, ids[:7]])
    out = unique_bias(dup, torch.cat([bias, bias[:7]]))
    assert torch.equal(out, torch.arange(1, 51).float() * 0.5)
    bad = torch.cat([bias, bias[:7]])
    bad[52] += 1.0
    with pytest.raises(ValueError, match=f"id {int(dup[52])} .* different biases"):
        unique_bias(dup, bad)


def test_catalogue_refusals():
    ids = torch.tensor([10, 20, 30], dtype=torch.int64)
    emb = torch.zeros((3, 128), dtype=torch.bfloat16)
    ItemCatalogue(ids, emb, None, torch.zeros(3))
    for bad in (torch.tensor([0.0, float("nan"), 1.0]), torch.tensor([0.0, float("inf"), 1.0]),
                torch.tensor([0.0, -float("inf"), 1.0]), torch.zeros(4), torch.zeros(2), torch.zeros(3, 1),
                torch.zeros(3, dtype=torch.float64), torch.zeros(3, dtype=torch.bfloat16),
                torch.zeros(3, dtype=torch.int32)):
        with pytest.raises(ValueError):
            ItemCatalogue(ids, emb, None, bad)
    with pytest.raises(ValueError):
        ItemCatalogue.from_embeddings(ids, emb, bias=torch.zeros(4))
    plain = ItemCatalogue(ids, emb)
    assert plain.bias is None
    for w in (1.0, 0.0, torch.zeros(1)):
        with pytest.raises(ValueError, match="no bias"):
            plain.topk(torch.zeros(1, 128), 1, bias_weight=w)  # a weight without a bias
    # the kernels' wrapper refuses a weight without a bias as well, before any kernel is looked for
    with pytest.raises(K.OperandError):
        K.retrieve_topk(torch.zeros(1, 128), emb, 1, bias_weight=1.0)
    with pytest.raises(K.OperandError):
        K.retrieve_topk_group(torch.zeros(1, 2, 128), emb, 1, bias_weight=torch.zeros(1))
