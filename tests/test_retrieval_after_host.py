"""CPU checks of the retrieval cursor's host layer: the new C ABI entry and struct, the checker the
GPU tests use (retrieval_after_case.py) pinned against a brute-force loop (cursors inside tie runs,
at +-inf and NaN, after_row at -1, N - 1, N and INT_MAX), the id-to-row mapping of
ItemCatalogue's id cursor, and the page arithmetic of the deep call.  No kernel is launched."""
import ctypes
import inspect
import math
import struct

import numpy as np
import pytest
import torch

from recommendations_amd import _lib
from recommendations_amd import kernels as K
from recommendations_amd.models.lthm.sequence.retrieval import ItemCatalogue
from retrieval_after_case import after_checker, after_eligible

INT_MAX = 2 ** 31 - 1
ALL32 = (1 << 32) - 1


def test_symbols_and_struct():
    lib = _lib.load()
    assert hasattr(lib, "lthm_retrieve_topk_after")
    protos = _lib.parse_header()
    assert protos["lthm_retrieve_topk_after"] == ("int", ["lthm_retrieve_desc*", "lthm_retrieve_excl*",
                                                          "lthm_retrieve_group*", "lthm_retrieve_tags*",
                                                          "lthm_retrieve_cursor*", "void*"])
    assert lib.lthm_abi_version() == 44  # additive: nothing existing changed layout or signature
    st = _lib.STRUCTS["lthm_retrieve_cursor"]
    assert [f[0] for f in st._fields_] == ["after_score", "after_row"] and ctypes.sizeof(st) == 16
    assert ctypes.sizeof(_lib.STRUCTS["lthm_retrieve_desc"]) == 104
    assert ctypes.sizeof(_lib.STRUCTS["lthm_retrieve_tags"]) == 16
    assert K.RETRIEVE_MAX_DEEP == 1024 and K.RETRIEVE_MAX_K == 128
    for fn in (K.retrieve_topk, K.retrieve_topk_group):
        p = inspect.signature(fn).parameters
        assert p["after_scores"].default is None and p["after_rows"].default is None and p["deep"].default is False
        assert p["after_scores"].kind is inspect.Parameter.KEYWORD_ONLY
    p = inspect.signature(ItemCatalogue.topk).parameters
    assert p["after_scores"].default is None and p["after_ids"].default is None
    from recommendations_amd.models.lthm.sequence.wrapper import LTHMModelWrapper
    assert inspect.signature(LTHMModelWrapper.retrieve).parameters["after"].default is None


def test_abi_refuses_half_a_cursor_struct():
    """With c, both pointers must be non-null and 4-byte aligned: refused on the host, before any
    launch."""
    lib = _lib.load()
    d = _lib.STRUCTS["lthm_retrieve_desc"]()
    buf = (ctypes.c_char * 4096)()
    base = (ctypes.addressof(buf) + 255) // 256 * 256
    d.items = d.q = d.scores = d.rows = d.workspace = base
    d.Q, d.N, d.k, d.q_dtype, d.normalize_q, d.slab_rows = 1, 1, 1, _lib.F32, 0, 0
    d.ws_bytes = 1 << 30
    c = _lib.STRUCTS["lthm_retrieve_cursor"]()
    g = _lib.STRUCTS["lthm_retrieve_group"]()
    for G in (1, 3):
        g.G = G
        for sc, row in ((0, 0), (base, 0), (0, base), (base + 2, base), (base, base + 1)):
            c.after_score, c.after_row = sc or None, row or None
            assert lib.lthm_retrieve_topk_after(ctypes.addressof(d), None, ctypes.addressof(g), None,
                                                ctypes.addressof(c), None) != 0


def f32(x):
    return struct.unpack("f", struct.pack("f", x))[0]


def brute(q, items, k, asc, arow, tags, filt, excl, trow):
    """The definition as Python loops over Python ints and floats (scores rounded to f32 for the
    cursor comparison, as the cursor itself is an f32)."""
    U, G, D = q.shape
    N = items.shape[0]
    qs, it = q.double().tolist(), items.double().tolist()
    out_rows, out_sc, ranks, tss = [], [], [], []
    for u in range(U):
        fa, fy, fn = (int(v) & ALL32 for v in filt[u])
        cs, cr = f32(float(asc[u])), int(arow[u])
        s, ok = [], []
        for j in range(N):
            sj = max(sum(a * b for a, b in zip(qs[u][g], it[j])) for g in range(G))
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


def test_checker_against_brute_force():
    g = torch.Generator().manual_seed(3)
    U, G, N, k = 12, 2, 29, 7
    q = torch.randint(-1, 2, (U, G, 128), generator=g).to(torch.bfloat16)
    items = torch.randint(-1, 2, (N, 128), generator=g).to(torch.bfloat16)
    items[5] = items[9] = items[20] = items[2]  # a tie run of four rows: 2, 5, 9, 20
    s = after_checker(q, items, k)[0]
    run = s[:, 2]
    assert (s[:, 5] == run).all() and (s[:, 20] == run).all()
    top = s.max(axis=1)
    # one cursor kind per user
    asc = np.array([run[0], run[1], run[2], run[3], run[4], np.inf, -np.inf, np.nan, top[8], top[9], run[10], 0.0],
                   dtype=np.float32)
    arow = np.array([5, 2, -1, N - 1, N, 3, 3, 3, INT_MAX, -1, INT_MAX, -(2 ** 31)], dtype=np.int64)
    tags = torch.randint(0, 4, (N,), generator=g).numpy().astype(np.int64)
    filt = np.zeros((U, 3), dtype=np.int64)
    filt[1] = [1, 0, 0]
    filt[9] = [0, 0, 2]
    excl = np.full((U, 2), -1)
    excl[0] = [9, N]  # the row after the cursor row inside the run
    excl[11] = [0, 1]
    trow = np.array([2, 20, -1, 4, N, 0, 1, 2, 3, 4, 5, 6])
    e = after_eligible(s, asc, arow)
    assert e[0, 9] and e[0, 20] and not e[0, 5] and not e[0, 2]       # inside the run: strictly behind row 5
    assert e[2, 2] and e[2, 5]                                          # after_row = -1 admits the whole run
    assert not e[3, [2, 5, 9, 20]].any() and not e[4, [2, 5, 9, 20]].any()  # N - 1 and N admit none of it
    assert e[5].all() and not e[6].any() and not e[7].any()             # +inf, -inf, NaN
    assert e[8].sum() == (s[8].astype(np.float32) < asc[8]).sum()       # INT_MAX: strictly lower scores only
    assert e[9].sum() == N                                              # the top score with row -1: everything
    b_sc, b_rows, b_rank, b_ts = brute(q, items, k, asc, arow, tags, filt, excl, trow)
    _, masked, sc, rows, rank, ts = after_checker(q, items, k, asc, arow, tags, filt, excl, trow)
    assert np.array_equal(rows, b_rows) and np.array_equal(sc.view(np.uint32), b_sc.view(np.uint32))
    assert np.array_equal(rank, b_rank) and np.array_equal(ts.view(np.uint32), b_ts.view(np.uint32))
    assert (rows[6] == -1).all() and (rows[7] == -1).all() and rank[6] == 0 and rank[7] == 0
    first = min(j for j in range(N) if j > 5 and j != 9 and np.float32(s[0, j]) == asc[0])
    assert rows[0, 0] == first <= 20 and 9 not in rows[0]  # row 9 is excluded; the run goes on behind it
    # without a cursor, and with a 2-D q, the checker is tags_checker
    from retrieval_tags_case import tags_checker
    a = after_checker(q[:, 0], items, k, None, None, tags, filt, excl, trow)
    b = tags_checker(q[:, 0], items, k, tags, filt, excl, trow)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    # -0 and +0 are one score
    assert after_eligible(np.array([[-0.0, 0.0, 0.0]]), np.array([0.0], dtype=np.float32), [0]).tolist() == [[False, True, True]]
    assert after_eligible(np.array([[0.0, 0.0]]), np.array([-0.0], dtype=np.float32), [-1]).tolist() == [[True, True]]


def test_paging_the_checker_concatenates():
    """Pages cut from the checker's own order with its last (score, row) as the next cursor are
    the full order: the property the kernels are held to."""
    g = torch.Generator().manual_seed(9)
    q = torch.randint(-1, 2, (4, 128), generator=g).to(torch.bfloat16)
    items = torch.randint(-1, 2, (50, 128), generator=g).to(torch.bfloat16)
    full = after_checker(q, items, 64)
    asc = np.full(4, np.inf, dtype=np.float32)
    arow = np.full(4, -1, dtype=np.int64)
    pages = []
    for _ in range(5):
        p = after_checker(q, items, 13, asc, arow)
        pages.append(p)
        asc, arow = p[2][:, -1].copy(), p[3][:, -1].astype(np.int64)
    assert np.array_equal(np.concatenate([p[3] for p in pages], axis=1)[:, :64], full[3][:, :64])
    assert (pages[4][3] == -1).all() and (pages[3][3][:, -2:] == -1).all()  # 50 rows: page 4 is 11 rows, page 5 empty


def test_id_cursor_maps_to_rows():
    ids = torch.tensor([10, 20, 30, 40, 60], dtype=torch.int64)
    emb = torch.zeros((5, 128), dtype=torch.bfloat16)
    cat = ItemCatalogue(ids, emb)
    after = torch.tensor([10, 30, 60, 25, 35, 50, 5, -7, 61, 2 ** 62, 0], dtype=torch.int64)
    got = cat.cursor_rows(after)
    assert got.dtype == torch.int32 and got.shape == after.shape
    #            present      | absent, between | below the first | above the last | the pad id
    assert got.tolist() == [0, 2, 4, 1, 2, 3, -1, -1, 4, 4, -1]
    for a, r in zip(after.tolist(), got.tolist()):  # "row > cursor row" is "id > after_id"
        assert [j > r for j in range(5)] == [int(i) > a for i in ids.tolist()]
    assert cat.cursor_rows(after.view(1, -1)).shape == (1, 11)
    with pytest.raises(ValueError):
        cat.topk(torch.zeros(1, 128), 1, after_scores=torch.zeros(1))           # one without the other
    with pytest.raises(ValueError):
        cat.topk(torch.zeros(1, 128), 1, after_ids=torch.zeros(1, dtype=torch.int64))
    with pytest.raises(ValueError):
        cat.topk(torch.zeros(1, 128), 1, after_scores=torch.zeros(1), after_ids=torch.zeros(1, dtype=torch.int32))


def test_deep_page_arithmetic():
    assert K.retrieve_deep_passes(1) == [1] and K.retrieve_deep_passes(128) == [128]
    assert K.retrieve_deep_passes(129) == [128, 1]
    assert K.retrieve_deep_passes(256) == [128, 128]
    assert K.retrieve_deep_passes(1000) == [128] * 7 + [104]
    assert K.retrieve_deep_passes(1024) == [128] * 8
    for k in (129, 256, 1000, 1024):
        p = K.retrieve_deep_passes(k)
        assert sum(p) == k and len(p) == -(-k // 128) and max(p) <= K.RETRIEVE_MAX_K and min(p) >= 1
    for bad in (0, -1, 1025, 4096):
        with pytest.raises(K.OperandError):
            K.retrieve_deep_passes(bad)
    # refused before any kernel is looked for, whatever the operands
    q, items = torch.zeros(2, 128), torch.zeros((5, 128), dtype=torch.bfloat16)
    with pytest.raises(K.OperandError):
        K.retrieve_topk(q, items, 1025, deep=True)
    with pytest.raises(K.OperandError):
        K.retrieve_topk_group(q[:, None], items, 1025, deep=True)
