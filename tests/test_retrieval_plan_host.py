"""CPU checks of the exact scan's workspace plan (csrc/retrieve.hip, RetrPlan): the four size
queries against a restatement of the layout, over a grid of sizes.  No kernel is launched."""
import itertools

from recommendations_amd import _lib

US = (1, 70, 4096, 20000)
GS = (1, 2, 3, 8)
NS = (1, 63, 3000, 2_000_000)
KS = (1, 128, 129, 1024)
SLABS = (0, 64, 4096)
XS = (0, 1, 1024)


def up256(x):
    return (x + 255) // 256 * 256


def plan_bytes(U, G, N, k, slab_rows, X):
    """The workspace of a scan of U users with G queries each, or -1: the queries as bf16 slots,
    the slabs' key lists, the slabs' counts, the sorted exclusion lists."""
    if not (1 <= G <= 8 and 1 <= k <= 1024 and 0 <= X <= 1024 and slab_rows >= 0):
        return -1
    gp = 1 << (G - 1).bit_length()  # slots per user
    S = U * gp
    if not (U >= 1 and S < 2 ** 31 and 1 <= N < 2 ** 31):
        return -1
    sr = slab_rows
    if sr == 0:
        nqt = -(-S // 64)
        want = 1 if nqt >= 256 else -(-256 // nqt)
        sr = max(-(-N // want), 1024 if k <= 128 else 4096)
        sr = -(-sr // 64) * 64
    nslab = -(-N // sr)
    if sr < 64 or sr % 64 or nslab > 65535:
        return -1
    stride = k if k <= 128 else (2048 if sr >= 2048 else max(sr, k))
    lists = up256(U * (X + 1) * 4) if X else 0
    return up256(S * 256) + up256(nslab * U * stride * 8) + up256(nslab * U * 4) + lists


def queries(lib, U, G, N, k, slab_rows, X):
    """(plain, excl, group, deep) as the library answers them; None where a query has no such argument"""
    plain = lib.lthm_retrieve_ws_bytes(U, N, k, slab_rows) if G == 1 and X == 0 else None
    excl = lib.lthm_retrieve_excl_ws_bytes(U, N, k, slab_rows, X) if G == 1 else None
    return (plain, excl, lib.lthm_retrieve_group_ws_bytes(U, G, N, k, slab_rows, X),
            lib.lthm_retrieve_deep_ws_bytes(U, G, N, k, slab_rows, X))


def test_size_queries_follow_the_layout():
    lib = _lib.load()
    seen = set()
    for U, G, N, k, slab_rows, X in itertools.product(US, GS, NS, KS, SLABS, XS):
        want = plan_bytes(U, G, N, k, slab_rows, X)
        assert want > 0  # every point of the grid is a valid call
        plain, excl, group, deep = queries(lib, U, G, N, k, slab_rows, X)
        at = (U, G, N, k, slab_rows, X)
        assert deep == want, at
        assert group == (want if k <= 128 else -1), at  # deep with k <= 128 equals group
        if excl is not None:  # group with G = 1 equals excl (X > 0: the excluding query refuses X = 0) ...
            assert excl == (group if X > 0 else -1), at
        if plain is not None:  # ... or plain
            assert plain == group, at
        seen.add(want)
    assert len(seen) > 200  # the grid does tell sizes apart


def test_size_queries_refuse():
    lib = _lib.load()
    U, N = 70, 3000
    assert plan_bytes(U, 3, N, 100, 0, 5) == lib.lthm_retrieve_deep_ws_bytes(U, 3, N, 100, 0, 5) > 0
    bad = [(U, 1, N, 0, 0, 0), (U, 1, N, 1025, 0, 0),  # k
           (U, 0, N, 10, 0, 0), (U, 9, N, 10, 0, 0),  # G
           (U, 1, N, 10, 0, 1025),  # X
           (U, 1, N, 10, -64, 0), (U, 1, N, 10, 65, 0),  # slab_rows
           (U, 1, 64 * 65535 + 1, 10, 64, 0), (U, 1, 64 * 65535 + 1, 300, 64, 0),  # more than 65535 slabs
           (1 << 28, 8, N, 10, 0, 0), (1 << 28, 8, N, 300, 0, 0), (1 << 31, 1, N, 10, 0, 0)]  # U gp >= 2^31
    for U_, G, N_, k, slab_rows, X in bad:
        assert plan_bytes(U_, G, N_, k, slab_rows, X) == -1
        for got in queries(lib, U_, G, N_, k, slab_rows, X):
            assert got in (None, -1), (U_, G, N_, k, slab_rows, X)
    # one slab fewer, one slot fewer: taken
    assert lib.lthm_retrieve_ws_bytes(U, 64 * 65535, 10, 64) == plan_bytes(U, 1, 64 * 65535, 10, 64, 0) > 0
    assert lib.lthm_retrieve_group_ws_bytes((1 << 28) - 1, 8, N, 10, 0, 0) == plan_bytes((1 << 28) - 1, 8, N, 10, 0, 0) > 0
