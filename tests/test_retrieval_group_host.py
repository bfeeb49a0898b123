"""CPU checks of the multi-head (grouped) retrieval's host layer: the new C ABI entries and
their workspace query, and the checker and host-merge helper the GPU tests use
(retrieval_group_case.py), pinned against a brute-force triple loop.  No kernel is launched."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from recommendations_amd import _lib
from recommendations_amd import kernels as K
from recommendations_amd.models.lthm.sequence.retrieval import ItemCatalogue
from retrieval_group_case import group_checker, host_merge


def test_symbols_exported():
    lib = _lib.load()
    assert K.RETRIEVE_MAX_GROUP == 8
    for name in ("lthm_retrieve_group_ws_bytes", "lthm_retrieve_topk_group"):
        assert hasattr(lib, name), name
        assert name in _lib.parse_header()
    assert lib.lthm_abi_version() == 44  # additive: nothing existing changed layout or signature
    st = _lib.STRUCTS["lthm_retrieve_group"]
    assert [f[0] for f in st._fields_] == ["G"] and ctypes.sizeof(st) == 4
    assert ctypes.sizeof(_lib.STRUCTS["lthm_retrieve_desc"]) == 104 and ctypes.sizeof(_lib.STRUCTS["lthm_retrieve_excl"]) == 16
    p = inspect.signature(K.retrieve_topk_group).parameters
    assert p["normalize_q"].default is True and p["exclude_rows"].default is None and p["target_rows"].default is None
    from recommendations_amd.models.lthm.sequence.wrapper import LTHMModelWrapper
    assert inspect.signature(LTHMModelWrapper.retrieve).parameters["heads"].default is None


def test_group_ws_bytes():
    lib = _lib.load()
    ws, base, excl = lib.lthm_retrieve_group_ws_bytes, lib.lthm_retrieve_ws_bytes, lib.lthm_retrieve_excl_ws_bytes
    shapes = [(256, 2_000_000, 100, 0), (4, 100, 5, 0), (1, 1, 1, 64), (33, 4101, 128, 64)]
    for U, N, k, sr in shapes:
        assert ws(U, 1, N, k, sr, 0) == base(U, N, k, sr) > 0  # G = 1 is the existing call
        for X in (1, 64, 1024):
            assert ws(U, 1, N, k, sr, X) == excl(U, N, k, sr, X) > 0
        for G in (0, 9, -1, 2 ** 20):
            assert ws(U, G, N, k, sr, 0) == -1 and ws(U, G, N, k, sr, 16) == -1, G
        for G in range(2, 9):
            gp = 1 << (G - 1).bit_length()
            b = ws(U, G, N, k, sr, 0)
            assert b >= U * gp * 256 + U * k * 8 + U * 4  # the padded queries, one slab's keys and counts
            assert ws(U, G, N, k, sr, 16) >= b + U * 17 * 4  # one sorted list per user, with its sentinel
            assert ws(U, G, N, k, sr, -1) == -1 and ws(U, G, N, k, sr, 1025) == -1
    # what the existing queries refuse (tests/test_retrieval_host.py's list), at every G
    for U, N, k, sr in [(0, 100, 10, 0), (-1, 100, 10, 0), (4, 0, 10, 0), (4, -5, 10, 0), (4, 2 ** 31, 10, 0),
                        (4, 100, 0, 0), (4, 100, 129, 0), (4, 100, 10, 63), (4, 100, 10, 100), (4, 100, 10, -64),
                        (4, 64 * 65536, 10, 64)]:
        for G in (1, 2, 3, 8):
            assert ws(U, G, N, k, sr, 0) == -1 and ws(U, G, N, k, sr, 16) == -1, (U, G, N, k, sr)
    assert ws(2 ** 28, 8, 100, 10, 0, 0) == -1  # 2^31 padded slots
    # monotone in U, with and without lists, wherever the slab count does not depend on U: a given
    # slab_rows, and slab_rows = 0 on a catalogue of one slab.  (On a long catalogue slab_rows = 0
    # cuts fewer slabs the more query tiles there are, for the plain call as well, so one more
    # tile can need less.)
    for G in (1, 2, 3, 6, 8):
        for N, sr in ((100_000, 64), (100_000, 1024), (1000, 0)):
            for X in (0, 128):
                by_u = [ws(U, G, N, 100, sr, X) for U in (1, 2, 8, 9, 33, 64, 65, 256, 4096)]
                assert all(v > 0 for v in by_u) and by_u == sorted(by_u) and by_u[0] < by_u[-1], (G, N, sr, X)


def test_topk_routes_3d_queries():
    g = torch.Generator().manual_seed(0)
    emb = torch.nn.functional.normalize(torch.randn(4, 128, generator=g), dim=-1).to(torch.bfloat16)
    cat = ItemCatalogue.from_embeddings(torch.tensor([50, -7, 3, 11]), emb)
    # both routes end in a kernel call, which has no CPU path
    with pytest.raises(RuntimeError, match="MI355X"):
        cat.topk(torch.zeros(3, 2, 128), 2)
    with pytest.raises(RuntimeError, match="MI355X"):
        cat.topk(torch.zeros(3, 128), 2)


def _brute(sg, k, excl, trow):
    """The definition, as loops over users, rows and heads: repeatedly take the best remaining
    non-excluded row (strict compare, rows ascending, so the lower row wins a tie)."""
    U, G, N = sg.shape
    rows = np.full((U, k), -1, dtype=np.int32)
    sc = np.full((U, k), -np.inf, dtype=np.float32)
    rank = np.full(U, -1, dtype=np.int32)
    for u in range(U):
        s = []
        for j in range(N):
            m = sg[u, 0, j]
            for g in range(1, G):
                if sg[u, g, j] > m:
                    m = sg[u, g, j]
            s.append(m)
        gone = {int(r) for r in excl[u] if 0 <= int(r) < N}
        taken = set()
        for slot in range(k):
            best = None
            for j in range(N):
                if j in gone or j in taken:
                    continue
                if best is None or s[j] > s[best]:
                    best = j
            if best is None:
                break
            taken.add(best)
            rows[u, slot], sc[u, slot] = best, np.float32(s[best])
        t = int(trow[u])
        if 0 <= t < N:
            rank[u] = sum(1 for j in range(N) if j != t and j not in gone and s[j] > s[t])
    return sc, rows, rank


def _case():
    g = torch.Generator().manual_seed(17)
    U, G, N = 5, 3, 70
    items = torch.randint(-2, 3, (N, 128), generator=g).to(torch.bfloat16)
    items[40] = items[7]  # ties
    items[55] = items[7]
    items[12] = items[30]
    q = torch.randint(-2, 3, (U, G, 128), generator=g).to(torch.bfloat16)
    return q, items


def test_checker_against_brute_force():
    q, items = _case()
    U, G, N = q.shape[0], q.shape[1], items.shape[0]
    sg = (q.double().reshape(U * G, 128) @ items.double().T).numpy().reshape(U, G, N)
    best = sg.max(1).argmax(1)
    trow = np.array([7, -1, 30, 3, N], dtype=np.int32)  # tied targets, none, plain, outside the catalogue
    excl = np.array([[int(best[0]), 7, 7, -1, N + 3],   # the best row, the target itself, junk
                     [2, 2, -1, 70, int(best[1])],
                     [12, 40, 2 ** 31 - 1, -7, 0],      # a row tied with the target
                     [-1, -1, -1, -1, -1],              # nothing valid
                     [1, 2, 3, 4, 5]], dtype=np.int64)
    for k in (1, 8, 70):
        sg2, s, masked, sc, rows, rank, tscore = group_checker(q, items, k, excl, trow)
        b_sc, b_rows, b_rank = _brute(sg, k, excl, trow)
        assert np.array_equal(sg2, sg) and np.array_equal(s, sg.max(1))
        assert np.array_equal(rows, b_rows) and np.array_equal(sc.view(np.uint32), b_sc.view(np.uint32)), k
        assert np.array_equal(rank, b_rank) and rank[1] == -1 and rank[4] == -1
        assert tscore[0] == np.float32(s[0, 7]) and np.isneginf(tscore[1]) and np.isneginf(tscore[4])
        for u in range(U):
            assert not set(rows[u].tolist()) & {int(r) for r in excl[u] if 0 <= r < N}
    # without lists the checker excludes nothing; fewer rows than k leave an empty tail
    _, s, masked, sc, rows, _, _ = group_checker(q, items, 8)
    assert np.array_equal(s, masked)
    _, _, _, sc, rows, _, _ = group_checker(q, items, 70, excl)
    for u in (0, 1, 2, 4):
        left = N - len({int(r) for r in excl[u] if 0 <= r < N})
        assert 0 < left < N
        assert (rows[u, :left] >= 0).all() and (rows[u, left:] == -1).all() and np.isneginf(sc[u, left:]).all()
    # user 0's target has two copies with the same score: the count is strict, so none of them counts
    assert s[0, 40] == s[0, 7] == s[0, 55]


def test_group_topk_lies_in_the_attaining_heads_topk():
    """Every row of the group's top-k is in the top-k of a head that attains its score: a row
    ahead of it in that head's order is ahead of it in the group's order as well.  This is what
    makes the merge of per-head top-k lists a reference for the grouped call."""
    q, items = _case()
    U, G, N = q.shape[0], q.shape[1], items.shape[0]
    k = 8
    sg, s, _, sc, rows, _, _ = group_checker(q, items, k)
    ar = np.arange(N)
    per_head = []
    for g in range(G):
        order = np.stack([np.lexsort((ar, -sg[u, g]))[:k] for u in range(U)])
        per_head.append((np.take_along_axis(sg[:, g], order, 1).astype(np.float32), order.astype(np.int32)))
    for u in range(U):
        for r in rows[u].tolist():
            g = int(np.argmax(sg[u, :, r]))
            assert sg[u, g, r] == s[u, r] and r in per_head[g][1][u].tolist(), (u, r, g)
    m_sc, m_rows = host_merge(per_head, k)
    assert np.array_equal(m_rows, rows) and np.array_equal(m_sc.view(np.uint32), sc.view(np.uint32))
    # the helper against its definition, by loops: duplicates across heads, ties, short lists with -1
    a = (np.array([[5.0, 3.0, 3.0, -np.inf]], dtype=np.float32), np.array([[4, 1, 9, -1]], dtype=np.int32))
    b = (np.array([[6.0, 3.0, 2.0, 1.0]], dtype=np.float32), np.array([[9, 0, 4, 7]], dtype=np.int32))
    m_sc, m_rows = host_merge([a, b], 6)
    assert m_rows.tolist() == [[9, 4, 0, 1, 7, -1]]
    assert m_sc.tolist() == [[6.0, 5.0, 3.0, 3.0, 1.0, -np.inf]]
    assert host_merge([a, b], 2)[1].tolist() == [[9, 4]]
