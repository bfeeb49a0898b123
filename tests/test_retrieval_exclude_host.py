"""CPU checks of the exclusion layer of the retrieval host code: the new C ABI entries and
their workspace query, ItemCatalogue's id-to-row mapping of exclude_ids, and the checker the
GPU tests use (retrieval_exclude_case.py), pinned against a brute-force double loop.  No kernel
is launched."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from recommendations_amd import _lib
from recommendations_amd import kernels as K
from recommendations_amd.kernels import RETRIEVE_MAX_EXCLUDE
from recommendations_amd.models.lthm.sequence.retrieval import ItemCatalogue
from retrieval_exclude_case import excl_checker


def test_symbols_exported():
    lib = _lib.load()
    assert RETRIEVE_MAX_EXCLUDE == 1024
    for name in ("lthm_retrieve_excl_ws_bytes", "lthm_retrieve_topk_excl"):
        assert hasattr(lib, name), name
        assert name in _lib.parse_header()
    assert lib.lthm_abi_version() == 44  # additive: nothing existing changed layout or signature
    assert "exclude_rows" in inspect.signature(K.retrieve_topk).parameters
    assert inspect.signature(K.retrieve_topk).parameters["exclude_rows"].default is None
    assert "exclude_ids" in inspect.signature(ItemCatalogue.topk).parameters
    from recommendations_amd.models.lthm.sequence.wrapper import LTHMModelWrapper
    assert inspect.signature(LTHMModelWrapper.retrieve).parameters["exclude_history"].default is False
    assert inspect.signature(LTHMModelWrapper.catalogue_metrics).parameters["exclude_seen"].default is False


def test_struct_parsed():
    st = _lib.STRUCTS["lthm_retrieve_excl"]
    assert [f[0] for f in st._fields_] == ["rows", "X"]
    assert ctypes.sizeof(st) == 16 and st.X.offset == 8
    # the descriptor of the plain call is the one it was
    assert ctypes.sizeof(_lib.STRUCTS["lthm_retrieve_desc"]) == 104


def test_excl_ws_bytes():
    lib = _lib.load()
    ws, base = lib.lthm_retrieve_excl_ws_bytes, lib.lthm_retrieve_ws_bytes
    for X in (0, -1, RETRIEVE_MAX_EXCLUDE + 1, 2 ** 40):
        assert ws(256, 2_000_000, 100, 0, X) == -1, X
    # every refusal of the base query (tests/test_retrieval_host.py's list)
    for Q, N, k, sr in [(0, 100, 10, 0), (-1, 100, 10, 0), (4, 0, 10, 0), (4, -5, 10, 0), (4, 2 ** 31, 10, 0),
                        (4, 100, 0, 0), (4, 100, 129, 0), (4, 100, 10, 63), (4, 100, 10, 100), (4, 100, 10, -64),
                        (4, 64 * 65536, 10, 64)]:
        assert base(Q, N, k, sr) == -1 and ws(Q, N, k, sr, 16) == -1, (Q, N, k, sr)
    for Q, N, k, sr in [(256, 2_000_000, 100, 0), (4, 100, 5, 0), (1, 1, 1, 64), (4, 2 ** 31 - 1, 128, 0)]:
        b = base(Q, N, k, sr)
        by_x = [ws(Q, N, k, sr, X) for X in (1, 2, 63, 64, 65, 512, 1023, 1024)]
        assert b > 0 and all(v > b for v in by_x), (Q, N, k, sr)
        assert by_x == sorted(by_x)  # monotone in X
        assert by_x[-1] >= b + Q * 1025 * 4  # the sorted lists with their sentinels fit behind the base
    assert ws(4096, 100_000, 100, 0, 512) > ws(4096, 100_000, 100, 0, 128) > ws(4096, 100_000, 100, 0, 1)


def test_exclude_ids_map_to_rows():
    g = torch.Generator().manual_seed(0)
    emb = torch.nn.functional.normalize(torch.randn(4, 128, generator=g), dim=-1).to(torch.bfloat16)
    cat = ItemCatalogue.from_embeddings(torch.tensor([50, -7, 3, 11]), emb)
    ids = torch.tensor([[3, 0, 50, 4], [0, 0, 0, 0], [11, -7, 2 ** 62, 11]])
    rows = cat.rows_of(ids)
    assert rows.dtype == torch.int32 and rows.shape == ids.shape
    assert rows.tolist() == [[1, -1, 3, -1], [-1, -1, -1, -1], [2, 0, -1, 2]]  # unknown ids and the pad id: -1
    q = torch.zeros(3, 128)
    with pytest.raises(ValueError, match="int64"):  # refused before anything reaches the device
        cat.topk(q, 2, exclude_ids=ids.to(torch.int32))
    with pytest.raises(ValueError, match="int64"):
        cat.topk(q, 2, exclude_ids=ids[0])
    with pytest.raises(RuntimeError, match="MI355X"):  # and the mapped rows go to the kernel call, which has no CPU path
        cat.topk(q, 2, exclude_ids=ids)


def _brute(s, k, excl, trow):
    """The definition, as loops: repeatedly take the best remaining non-excluded row (strict
    compare, rows ascending, so the lower row wins a tie)."""
    Q, N = s.shape
    rows = np.full((Q, k), -1, dtype=np.int32)
    sc = np.full((Q, k), -np.inf, dtype=np.float32)
    rank = np.full(Q, -1, dtype=np.int32)
    for i in range(Q):
        gone = {int(r) for r in excl[i] if 0 <= int(r) < N}
        taken = set()
        for slot in range(k):
            best = None
            for j in range(N):
                if j in gone or j in taken:
                    continue
                if best is None or s[i, j] > s[i, best]:
                    best = j
            if best is None:
                break
            taken.add(best)
            rows[i, slot], sc[i, slot] = best, np.float32(s[i, best])
        t = int(trow[i])
        if 0 <= t < N:
            c = 0
            for j in range(N):
                if j != t and j not in gone and s[i, j] > s[i, t]:
                    c += 1
            rank[i] = c
    return sc, rows, rank


def test_checker_against_brute_force():
    g = torch.Generator().manual_seed(3)
    N, Q = 9, 3
    items = torch.randint(-2, 3, (N, 128), generator=g).to(torch.bfloat16)
    items[5] = items[2]  # ties
    items[7] = items[2]
    q = torch.randint(-2, 3, (Q, 128), generator=g).to(torch.bfloat16)
    s = (q.double() @ items.double().T).numpy()
    best = np.argmax(s, axis=1)
    trow = np.array([4, -1, 2], dtype=np.int32)
    # a duplicate, a -1, an out-of-range entry and (queries 0 and 2) the target itself
    excl = np.array([[int(best[0]), 4, 4, -1, N + 3],
                     [2, 2, -1, 9, int(best[1])],
                     [2, 5, 2 ** 31 - 1, -7, 0]], dtype=np.int64)
    for k in (1, 4, 9):
        s2, masked, sc, rows, rank = excl_checker(q, items, k, excl, trow)
        b_sc, b_rows, b_rank = _brute(s, k, excl, trow)
        assert np.array_equal(s2, s)
        assert np.array_equal(rows, b_rows) and np.array_equal(sc.view(np.uint32), b_sc.view(np.uint32)), k
        assert np.array_equal(rank, b_rank) and rank[1] == -1
        for i in range(Q):
            assert not set(rows[i].tolist()) & {int(r) for r in excl[i] if 0 <= r < N}
    # fewer rows remain than k: the tail is empty
    _, _, sc, rows, _ = excl_checker(q, items, 9, excl, trow)
    for i in range(Q):
        left = N - len({int(r) for r in excl[i] if 0 <= r < N})
        assert 0 < left < N
        assert (rows[i, :left] >= 0).all() and (rows[i, left:] == -1).all() and np.isneginf(sc[i, left:]).all()
    # query 2 excludes the tied rows 2 and 5: their third copy, row 7, stays
    assert 7 in rows[2].tolist() and 2 not in rows[2].tolist() and 5 not in rows[2].tolist()
