"""Multi-head retrieval: top-K by the best score over a user's queries (lthm_retrieve_topk_group,
K.retrieve_topk_group, ItemCatalogue.topk with a 3-D q, LTHMModelWrapper.retrieve's heads,
torch.ops.lthm.retrieve_topk_group) against the checker of retrieval_group_case.py, which
test_retrieval_group_host.py pins on the CPU.

Definition under test: s[u, j] = max_g s_g[u, j] over the user's G <= 8 queries, -inf at the
user's excluded rows (one list per user); the k best by (score descending, row ascending);
target_score[u] = max_g of the per-head target dots and rank[u] = #{j != target, j not excluded :
s[u, j] > target_score[u]}, -1 for an absent target.  G = 1 is the plain call, and the order of a
user's heads changes no bit.

Exact cases: the integer catalogue of the exclusion tests (1,367 random rows in {-2..2} three
times each at permuted positions, N = 4,101) and integer queries, normalize_q=False.  Every
partial sum is an integer below 2^10, so scores, rows, rank and target_score must match the
checker bit for bit, and ties occur at every rank.  Every case runs at slab_rows = 0 (one slab)
and 64 (65 slabs, the last partial).  Each constructed case first asserts, on the checker alone,
that it has the property it is there for.

Float case: unit vectors, f32 queries with bf16-representable values, normalize_q=True; the eps =
1e-5 rules of the plain and excluding tests (f32 accumulation of 128 products of unit vectors errs
by at most 128 * 2^-24 <= 7.7e-6; a maximum over heads errs by no more than its operands)."""
from typing import Optional, Tuple

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from retrieval_exclude_case import valid_rows
from retrieval_group_case import group_checker, host_merge

pytestmark = pytest.mark.gpu

EPS = 1e-5
D = 128
N_INT = 4101
SLABS = [0, 64]
U_MAX, G_MAX = 33, 8
NEG_INF_BITS = np.array([-np.inf], dtype=np.float32).view(np.uint32)[0]
_CACHE = {}


def int_case():
    """items [4101, 128] bf16 and queries [33, 8, 128] f32, small integers."""
    if "int" not in _CACHE:
        g = torch.Generator().manual_seed(1234)
        base = torch.randint(-2, 3, (1367, D), generator=g)
        perm = torch.randperm(3 * 1367, generator=g)
        items = base.repeat(3, 1)[perm].to(torch.bfloat16)
        q = torch.randint(-2, 3, (U_MAX, G_MAX, D), generator=g).float()
        _CACHE["int"] = (q, items)
    return _CACHE["int"]


def targets(U, N):
    trow = ((torch.arange(U) * 7919 + 3) % N).to(torch.int32)
    trow[::5] = -1
    return trow


def pad(lists, X, fill=-1):
    out = np.full((len(lists), X), fill, dtype=np.int64)
    for i, lst in enumerate(lists):
        assert len(lst) <= X
        out[i, :len(lst)] = lst
    return out


def run(dev, q, items, k, slab_rows, excl=None, trow=None, normalize_q=False):
    """One grouped call; the outputs as numpy arrays (scores as their bits)."""
    from recommendations_amd import kernels as K
    xr = None if excl is None else torch.from_numpy(np.asarray(excl, dtype=np.int64)).to(torch.int32).contiguous().to(dev)
    scores, rows, rank, tscore = K.retrieve_topk_group(q.contiguous().to(dev), items.to(dev), k, normalize_q=normalize_q,
                                                       slab_rows=slab_rows, exclude_rows=xr,
                                                       target_rows=None if trow is None else trow.to(dev))
    assert scores.shape == (q.shape[0], k) and rows.shape == (q.shape[0], k)
    out = [scores.cpu().numpy().view(np.uint32), rows.cpu().numpy()]
    if trow is not None:
        assert rank.shape == (q.shape[0],) and tscore.shape == (q.shape[0],)
        out += [rank.cpu().numpy(), tscore.cpu().numpy().view(np.uint32)]
    return out


def run_plain(dev, q, items, k, slab_rows, excl=None, trow=None, normalize_q=False):
    from recommendations_amd import kernels as K
    xr = None if excl is None else torch.from_numpy(np.asarray(excl, dtype=np.int64)).to(torch.int32).contiguous().to(dev)
    scores, rows, rank, tscore = K.retrieve_topk(q.contiguous().to(dev), items.to(dev), k, normalize_q=normalize_q,
                                                 slab_rows=slab_rows, exclude_rows=xr,
                                                 target_rows=None if trow is None else trow.to(dev))
    out = [scores.cpu().numpy().view(np.uint32), rows.cpu().numpy()]
    if trow is not None:
        out += [rank.cpu().numpy(), tscore.cpu().numpy().view(np.uint32)]
    return out


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def expect_exact(dev, q, items, k, slab_rows, excl=None, trow=None, ref=None):
    """Run and compare with the checker bit for bit; returns (outputs, checker results)."""
    if ref is None:
        ref = group_checker(q.to(torch.bfloat16), items, k, excl, None if trow is None else trow.numpy())
    _, _, _, e_sc, e_rows, e_rank, e_ts = ref
    got = run(dev, q, items, k, slab_rows, excl, trow)
    if excl is not None:
        for u in range(q.shape[0]):  # no excluded row comes back
            assert not set(got[1][u].tolist()) & set(valid_rows(excl[u], items.shape[0]).tolist()), u
    assert np.array_equal(got[1], e_rows[:, :k]), (slab_rows, k)
    assert np.array_equal(got[0], e_sc[:, :k].view(np.uint32)), (slab_rows, k)
    if trow is not None:
        assert np.array_equal(got[2], e_rank), slab_rows
        assert np.array_equal(got[3], e_ts.view(np.uint32)), slab_rows
    return got, ref


# ------------------------------------------------------------------ 1. bit-exact against the checker
@pytest.mark.parametrize("slab_rows", SLABS)
@pytest.mark.parametrize("U", [1, 8, 9, 33])
@pytest.mark.parametrize("G", [1, 2, 3, 4, 6, 8])
def test_exact(dev, G, U, slab_rows):
    """U = 8 at G = 8 fills one tile of 64 slots exactly, U = 9 spills one group into a second,
    partial tile; G = 3 and 6 have pad slots."""
    q, items = int_case()
    qs = q[:U, :G].contiguous()
    trow = targets(U, N_INT)
    key = ("exact", G, U)
    if key not in _CACHE:  # the checker's order does not depend on k: computed once at 128
        _CACHE[key] = group_checker(qs.to(torch.bfloat16), items, 128, None, trow.numpy())
    for k in (1, 100, 128):
        expect_exact(dev, qs, items, k, slab_rows, None, trow, ref=_CACHE[key])


# ------------------------------------------------------------------ 2. every head can win
@pytest.mark.parametrize("slab_rows", SLABS)
@pytest.mark.parametrize("G", [2, 4, 7, 8])
def test_every_head_can_win(dev, G, slab_rows):
    """For every user and head g there are rows that only head g scores best, inside the top-k
    and outside it above the target: a wrong xor distance or a missing step of the cross-lane
    maximum loses those of some head."""
    q, items = int_case()
    U, k = 9, 100
    qs = q[:U, :G].clone()
    qs[qs == 0] = 1.0
    items = items.clone()
    for u in range(U):
        for g in range(G):  # head g's best possible row: no other head of the user comes near it
            items[50 + 50 * (G_MAX * u + g)] = (2 * torch.sign(qs[u, g])).to(torch.bfloat16)
    trow = torch.zeros(U, dtype=torch.int32)
    sg, s, _, _, rows, _, _ = group_checker(qs.to(torch.bfloat16), items, k)
    for u in range(U):
        trow[u] = int(np.argsort(s[u])[N_INT // 4])  # a low target: most rows count in its rank
    for u in range(U):
        top = set(rows[u].tolist())
        for g in range(G):
            others = np.delete(sg[u], g, axis=0).max(0)
            only_g = np.nonzero(sg[u, g] > others)[0]  # head g is the unique maximiser
            assert any(int(j) in top for j in only_g), (u, g)
            outside = [int(j) for j in only_g if int(j) not in top and s[u, j] > s[u, int(trow[u])]]
            # without head g these rows would drop out of the count: their other heads score below the target
            assert any(others[j] <= s[u, int(trow[u])] for j in outside), (u, g)
    expect_exact(dev, qs, items, k, slab_rows, None, trow)


# ------------------------------------------------------------------ 3. pad slots
@pytest.mark.parametrize("slab_rows", SLABS)
@pytest.mark.parametrize("G", [3, 5, 6, 7])
def test_pad_slots_with_negative_scores(dev, G, slab_rows):
    """Every score of every group is negative: a zero-filled pad slot would score 0 everywhere and
    win every maximum."""
    g = torch.Generator().manual_seed(G)
    U = 9
    items = torch.randint(0, 3, (N_INT, D), generator=g).to(torch.bfloat16)
    items[:, 0] = 1
    qs = -torch.randint(1, 3, (U, G, D), generator=g).float()
    trow = targets(U, N_INT)
    ref = group_checker(qs.to(torch.bfloat16), items, 50, None, trow.numpy())
    assert ref[1].max() < 0
    expect_exact(dev, qs, items, 50, slab_rows, None, trow, ref=ref)


# ------------------------------------------------------------------ 4. no leak between neighbours
@pytest.mark.parametrize("slab_rows", SLABS)
@pytest.mark.parametrize("G", [2, 3, 5, 8])
def test_no_leak_between_neighbours(dev, G, slab_rows):
    """User u owns five rows that its first and its last head score far above everything else,
    and that no other user scores high.  A maximum that reached into a neighbour's lanes (its
    real or its pad slots) would put the neighbour's rows into u's list."""
    q, items = int_case()
    U, k = 24, 5
    qs = q[:U, :G].clone()
    qs[qs == 0] = 1.0
    items = items.clone()
    own = {}
    for u in range(U):
        own[u] = [100 + 160 * u + 7 * i for i in range(5)]
        for i, r in enumerate(own[u]):
            items[r] = (2 * torch.sign(qs[u, 0 if i % 2 == 0 else G - 1])).to(torch.bfloat16)
    ref = group_checker(qs.to(torch.bfloat16), items, k)
    s = ref[1]
    for u in range(U):
        assert sorted(ref[4][u].tolist()) == own[u]
        for v in range(U):
            if v != u:  # u's rows are nowhere near v's list
                assert s[v, own[u]].max() < s[v, ref[4][v, -1]] - 50
    got, _ = expect_exact(dev, qs, items, k, slab_rows, ref=ref)
    for u in range(U):
        for v in (u - 1, u + 1):
            if 0 <= v < U:
                assert not set(got[1][u].tolist()) & set(own[v])


# ------------------------------------------------------------------ 5. G = 1 and identical copies
@pytest.mark.parametrize("slab_rows", SLABS)
@pytest.mark.parametrize("with_excl", [False, True])
def test_copies_equal_plain_call(dev, with_excl, slab_rows):
    q, items = int_case()
    U, k = 33, 100
    q1 = q[:U, 0].contiguous()
    trow = targets(U, N_INT)
    g = torch.Generator().manual_seed(77)
    excl = None
    if with_excl:
        plain_rows = run_plain(dev, q1, items, 20, slab_rows)[1]
        excl = np.concatenate([plain_rows[:, :20:2].astype(np.int64),
                               torch.randint(-1, N_INT, (U, 30), generator=g).numpy()], axis=1)
    want = run_plain(dev, q1, items, k, slab_rows, excl, trow)
    for G in (1, 2, 3, 5, 8):
        got = run(dev, q1[:, None, :].expand(U, G, D), items, k, slab_rows, excl, trow)
        assert same(got, want), G
    # float queries through the normalisation: the grouped preparation is the plain one, bit for bit
    qf = torch.randn(U, D, generator=g)
    itf = F.normalize(torch.randn(3000, D, generator=g), dim=-1).to(torch.bfloat16)
    tr = targets(U, 3000)
    xf = None if excl is None else np.minimum(excl, 2999)
    for dt in (torch.float32, torch.bfloat16):
        want = run_plain(dev, qf.to(dt), itf, k, slab_rows, xf, tr, normalize_q=True)
        for G in (1, 3, 8):
            got = run(dev, qf.to(dt)[:, None, :].expand(U, G, D), itf, k, slab_rows, xf, tr, normalize_q=True)
            assert same(got, want), (G, dt)


# ------------------------------------------------------------------ 6. head order invariance
@pytest.mark.parametrize("slab_rows", SLABS)
@pytest.mark.parametrize("G", [3, 6, 8])
def test_head_order_invariance(dev, G, slab_rows):
    q, items = int_case()
    U, k = 33, 100
    qs = q[:U, :G].contiguous()
    g = torch.Generator().manual_seed(G)
    trow = targets(U, N_INT)
    excl = torch.randint(-1, N_INT, (U, 40), generator=g).numpy()
    a = run(dev, qs, items, k, slab_rows, excl, trow)
    shuffled = torch.stack([qs[u, torch.randperm(G, generator=g)] for u in range(U)])
    assert not torch.equal(shuffled, qs)
    assert same(run(dev, shuffled, items, k, slab_rows, excl, trow), a)
    assert same(run(dev, qs.flip(1), items, k, slab_rows, excl, trow), a)  # the pad slots repeat another head now
    # float operands: the maximum of the same six f32 scores, whatever their order
    qf = torch.randn(U, G, D, generator=g)
    a = run(dev, qf, items, k, slab_rows, excl, trow, normalize_q=True)
    assert same(run(dev, qf.flip(1), items, k, slab_rows, excl, trow, normalize_q=True), a)


# ------------------------------------------------------------------ 7. the plain kernel as reference
def test_float_against_plain_calls_and_checker(dev):
    U, G, N, k = 33, 6, 4101, 100
    g = torch.Generator().manual_seed(47)
    items = F.normalize(torch.randn(N, D, generator=g), dim=-1).to(torch.bfloat16)
    q = F.normalize(torch.randn(U, G, D, generator=g), dim=-1).to(torch.bfloat16).float()
    assert torch.equal(F.normalize(q, dim=-1).to(torch.bfloat16).float(), q)  # the kernel's bf16 operand is q itself
    trow = ((torch.arange(U) * 104729 + 11) % N).to(torch.int32)
    trow[3::7] = -1
    sg, s, _, _, _, e_rank, e_ts = group_checker(q.to(torch.bfloat16), items, k, None, trow.numpy())
    for u in range(U):  # a condition on the checker's own scores, before the GPU's are looked at
        kth = np.sort(s[u])[::-1][k - 1]
        assert int((np.abs(s[u] - kth) <= EPS).sum()) <= 4, "too many catalogue rows within eps of the k-th score"
    for slab_rows in SLABS:
        got = run(dev, q, items, k, slab_rows, None, trow, normalize_q=True)
        heads = [run_plain(dev, q[:, h], items, k, slab_rows, None, trow, normalize_q=True) for h in range(G)]
        m_sc, m_rows = host_merge([(h[0].view(np.float32), h[1]) for h in heads], k)
        assert np.array_equal(got[1], m_rows) and np.array_equal(got[0], m_sc.view(np.uint32)), slab_rows
        ts = np.stack([h[3].view(np.float32) for h in heads]).max(0)  # the best of the plain target dots
        assert np.array_equal(got[3], ts.view(np.uint32))
        g_scores, g_rows, g_rank = got[0].view(np.float32), got[1], got[2]
        for u in range(U):
            r = g_rows[u]
            assert (r >= 0).all() and (r < N).all() and len(set(r.tolist())) == k
            assert np.abs(g_scores[u].astype(np.float64) - s[u, r]).max() <= EPS
            assert (np.diff(g_scores[u]) <= 0).all()
            kth = np.sort(s[u])[::-1][k - 1]
            assert set(np.nonzero(s[u] > kth + EPS)[0].tolist()) <= set(r.tolist())
            assert (s[u, r] >= kth - EPS).all()
            t = int(trow[u])
            if t >= 0:
                near = int((np.abs(np.delete(s[u], t) - s[u, t]) <= EPS).sum())
                assert abs(int(g_rank[u]) - int(e_rank[u])) <= near, (u, int(g_rank[u]), int(e_rank[u]), near)
                assert abs(float(got[3].view(np.float32)[u]) - float(s[u, t])) <= EPS
            else:
                assert int(g_rank[u]) == -1


# ------------------------------------------------------------------ 8. exclusion
@pytest.mark.parametrize("slab_rows", SLABS)
def test_exclusion(dev, slab_rows):
    from recommendations_amd import kernels as K
    q, items = int_case()
    U, G, k = 9, 4, 20
    qs = q[:U, :G].clone()
    qs[qs == 0] = -1.0
    items = items.clone()
    star = [1000 + 37 * u for u in range(U)]
    for u in range(U):  # user u's best row by far, through head 2 alone
        items[star[u]] = (2 * torch.sign(qs[u, 2])).to(torch.bfloat16)
    sg, s, _, _, rows, _, _ = group_checker(qs.to(torch.bfloat16), items, k)
    for u in range(U):
        assert rows[u, 0] == star[u] and sg[u, 2, star[u]] > np.delete(sg[u, :, star[u]], 2).max() + 50
    trow = targets(U, N_INT)
    lists = [[star[u], -1, N_INT + 3] if u % 2 == 0 else [-1, -1, N_INT] for u in range(U)]
    got, _ = expect_exact(dev, qs, items, k, slab_rows, pad(lists, 3), trow)
    for u in range(U):
        assert (star[u] in got[1][u].tolist()) == (u % 2 == 1)
    # a user whose whole group top-k is excluded: ranks 128..255 of the unfiltered order come back
    ref = group_checker(qs.to(torch.bfloat16), items, 128)
    order = np.stack([np.lexsort((np.arange(N_INT), -ref[1][u])) for u in range(U)])
    assert np.array_equal(order[:, :128], ref[4])
    got, _ = expect_exact(dev, qs, items, 128, slab_rows, pad([order[u, :128].tolist() for u in range(U)], 130), trow)
    assert np.array_equal(got[1], order[:, 128:256].astype(np.int32))
    # fewer than k rows left, and none
    g = torch.Generator().manual_seed(9)
    small = items[:70].contiguous()
    excl = np.stack([torch.randperm(70, generator=g)[:65].numpy() for _ in range(U)])
    got, _ = expect_exact(dev, qs, small, 10, slab_rows, excl, targets(U, 70))
    assert (got[1][:, :5] >= 0).all() and (got[1][:, 5:] == -1).all() and (got[0][:, 5:] == NEG_INF_BITS).all()
    excl = np.stack([torch.randperm(7, generator=g).numpy() for _ in range(U)])
    t7 = torch.tensor([3, -1, 0, 6, 2, 1, 5, 4, -1], dtype=torch.int32)
    got, _ = expect_exact(dev, qs, small[:7].contiguous(), 10, slab_rows, excl, t7)
    assert (got[1] == -1).all() and got[2].tolist() == [0, -1, 0, 0, 0, 0, 0, 0, -1]
    # one list per user: a list per head is refused
    per_head = torch.full((U * G, 3), -1, dtype=torch.int32, device=dev)
    with pytest.raises(K.OperandError):
        K.retrieve_topk_group(qs.to(dev), items.to(dev), k, exclude_rows=per_head)


# ------------------------------------------------------------------ 9. rank
@pytest.mark.parametrize("slab_rows", SLABS)
@pytest.mark.parametrize("G", [3, 8])
def test_rank(dev, G, slab_rows):
    q, items = int_case()
    U = 33
    qs = q[:U, :G].contiguous()
    trow = targets(U, N_INT)  # every fifth absent
    sg, s, _, _, _, _, _ = group_checker(qs.to(torch.bfloat16), items, 1)
    lists, by_other_head, tied, moved = [], 0, 0, 0
    for u in range(U):
        t = int(trow[u])
        lst = []
        if t >= 0:
            by_other_head += int(sg[u, 0, t] < s[u, t])        # another head than 0 attains the target's score
            tied += int((s[u] == s[u, t]).sum() >= 3)          # its two copies score the same: the count is strict
            if u % 3 == 0:
                lst.append(t)                                   # the target inside its own list
            if u % 3 == 1:
                above = np.nonzero(s[u] > s[u, t])[0]
                if len(above) > 1:
                    lst += [int(above[0]), int(above[-1])]      # two rows that score above the target
                    moved += 1
        lists.append(lst)
    assert by_other_head > 10 and tied > 10 and moved > 5 and (trow.numpy() < 0).sum() > 5
    got, ref = expect_exact(dev, qs, items, 10, slab_rows, pad(lists, 4), trow)
    plain, _ = expect_exact(dev, qs, items, 10, slab_rows, None, trow)
    assert np.array_equal(got[3], plain[3])  # target_score does not know about the lists
    d = plain[2] - got[2]
    assert (d >= 0).all() and (got[2][trow.numpy() < 0] == -1).all()
    for u in range(1, U, 3):
        if len(lists[u]) == 2:
            assert d[u] == 2
    # the grouped rank is not any per-head rank: no head sees as few rows above the target as the group
    heads = [run_plain(dev, qs[:, h], items, 1, slab_rows, None, trow)[2] for h in range(G)]
    assert any((plain[2][u] != np.array([h[u] for h in heads])).all() for u in range(U) if int(trow[u]) >= 0)


# ------------------------------------------------------------------ 10. determinism
@pytest.mark.parametrize("slab_rows", SLABS)
def test_deterministic(dev, slab_rows):
    q, items = int_case()
    g = torch.Generator().manual_seed(5)
    excl = np.stack([torch.randperm(N_INT, generator=g)[:512].numpy() for _ in range(U_MAX)])
    trow = targets(U_MAX, N_INT)
    a = run(dev, q[:, :6], items, 100, slab_rows, excl, trow)
    b = run(dev, q[:, :6], items, 100, slab_rows, excl, trow)  # a fresh workspace and fresh outputs
    assert same(a, b)


# ------------------------------------------------------------------ 11. refusals
def test_refusals(dev):
    from recommendations_amd import kernels as K
    assert K.RETRIEVE_MAX_GROUP == 8
    items = torch.zeros((100, D), dtype=torch.bfloat16, device=dev)
    q = torch.zeros((4, 3, D), device=dev)
    ok_x = torch.full((4, 8), -1, dtype=torch.int32, device=dev)
    ok_t = torch.zeros(4, dtype=torch.int32, device=dev)
    K.retrieve_topk_group(q, items, 5, exclude_rows=ok_x, target_rows=ok_t)
    bad = [dict(q=torch.zeros((4, 0, D), device=dev)),                         # G = 0
           dict(q=torch.zeros((4, 9, D), device=dev)),                         # G = 9
           dict(q=torch.zeros((4, D), device=dev)),                            # a 2-D q
           dict(q=torch.zeros((4, 3, 64), device=dev)),                        # not 128 wide
           dict(target_rows=torch.zeros(12, dtype=torch.int32, device=dev)),   # [U G]
           dict(target_rows=torch.zeros((4, 3), dtype=torch.int32, device=dev)),
           dict(target_rows=ok_t.long()),
           dict(exclude_rows=torch.full((12, 8), -1, dtype=torch.int32, device=dev)),  # [U G, X]
           dict(exclude_rows=ok_x.view(-1)),
           dict(exclude_rows=ok_x.long()),
           dict(exclude_rows=torch.full((4, 1025), -1, dtype=torch.int32, device=dev)),
           dict(k=129), dict(k=0), dict(slab_rows=100)]
    for kw in bad:
        args = dict(q=q, k=5)
        args.update(kw)
        with pytest.raises(K.OperandError):
            K.retrieve_topk_group(args.pop("q"), items, args.pop("k"), **args)
    # the raw ABI refuses before any launch; g == NULL and G = 1 are the existing call
    import ctypes
    from recommendations_amd import _lib
    lib = _lib.load()
    scores = torch.full((4, 5), 123.0, device=dev)
    rows = torch.full((4, 5), 77, dtype=torch.int32, device=dev)
    need = lib.lthm_retrieve_group_ws_bytes(4, 3, 100, 5, 0, 8)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    d = _lib.STRUCTS["lthm_retrieve_desc"]()
    d.items, d.q, d.scores, d.rows = items.data_ptr(), q.data_ptr(), scores.data_ptr(), rows.data_ptr()
    d.workspace, d.ws_bytes = ws.data_ptr(), need
    d.Q, d.N, d.k, d.q_dtype, d.normalize_q, d.slab_rows = 4, 100, 5, _lib.F32, 1, 0
    x = _lib.STRUCTS["lthm_retrieve_excl"]()
    x.rows, x.X = ok_x.data_ptr(), 8
    grp = _lib.STRUCTS["lthm_retrieve_group"]()
    stream = torch.cuda.current_stream().cuda_stream
    call = lambda: lib.lthm_retrieve_topk_group(ctypes.addressof(d), ctypes.addressof(x), ctypes.addressof(grp), stream)
    for G in (0, 9, -1):
        grp.G = G
        assert call() != 0
    grp.G = 3
    d.ws_bytes = lib.lthm_retrieve_group_ws_bytes(4, 3, 100, 5, 0, 0)  # covers the call without lists only
    assert call() != 0
    d.ws_bytes, d.k = need, 129
    assert call() != 0
    d.k = 5
    torch.cuda.synchronize()
    assert bool((scores == 123.0).all()) and bool((rows == 77).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((rows[:, 0] == 0).all())  # all scores 0: row 0 leads
    rows.fill_(77)
    grp.G = 1  # q read as [4, 128]
    assert call() == 0
    assert lib.lthm_retrieve_topk_group(ctypes.addressof(d), None, None, stream) == 0
    torch.cuda.synchronize()
    assert bool((rows[:, 0] == 0).all())


# ------------------------------------------------------------------ 12. model level
def _model_case(dev):
    """A tiny model with the default six lookahead heads and 128-wide towers, one forward."""
    if "model" not in _CACHE:
        from recommendations_amd.data import synthetic_lthm_batch
        from recommendations_amd.models.lthm.builder import LTHMModelBuilder
        from recommendations_amd.models.lthm.config import lthm_config
        from recommendations_amd.models.lthm.sequence.retrieval import build_catalogue
        torch.manual_seed(0)
        cfg = lthm_config(T=48, d=128, n_layers=2, n_head=2, cat_features=2, cat_vocab=10_000, item_vocab=10_000,
                          log_q_buckets=1 << 16)
        m = LTHMModelBuilder(None, cfg).build().to(dev).eval()
        batch = synthetic_lthm_batch(32, 48, n_cat=2, seed=7)
        b = {k: v.to(dev) for k, v in batch.items()}
        with torch.no_grad():
            out = m(b)
        ids = batch["product_ids"].reshape(-1)
        g = torch.Generator().manual_seed(5)
        extra = torch.randint(1, 2 ** 62, (300,), generator=g)
        assert not bool(torch.isin(extra, ids).any())
        cat = build_catalogue(m, torch.cat([extra, ids[ids != 0]]), chunk=128)
        _CACHE["model"] = (m, b, out, cat)
    return _CACHE["model"]


def test_wrapper_retrieve_heads(dev):
    m, b, out, cat = _model_case(dev)
    k, heads = 20, [0, 2, 3]
    assert len(m._lookahead) == 6
    y = out["next_token_emb"]
    q = y[:, -1, heads].contiguous()
    if q.dtype not in (torch.float32, torch.bfloat16):
        q = q.float()
    assert q.dim() == 3 and q.shape[1] == 3
    res = m.retrieve(b, cat, k, heads=heads)
    item_ids, scores, _, _ = cat.topk(q, k)
    assert res["item_ids"].dtype == torch.int64 and res["item_ids"].shape == (y.shape[0], k)
    assert torch.equal(res["item_ids"], item_ids) and torch.equal(res["scores"], scores)
    assert torch.equal(m.retrieve(b, cat, k, head=5, heads=heads)["item_ids"], item_ids)  # head is ignored
    # the lists follow the definition: the eps rules against the fp64 checker
    q_bf = F.normalize(q.float().cpu(), dim=-1).to(torch.bfloat16)
    _, s, _, _, _, _, _ = group_checker(q_bf, cat.emb.cpu(), k)
    g_rows = cat.rows_of(res["item_ids"]).cpu().numpy()
    for i in range(q.shape[0]):
        kth = np.sort(s[i])[::-1][k - 1]
        assert set(np.nonzero(s[i] > kth + EPS)[0].tolist()) <= set(g_rows[i].tolist())
        assert (s[i, g_rows[i]] >= kth - EPS).all()
        assert np.abs(res["scores"][i].cpu().numpy().astype(np.float64) - s[i, g_rows[i]]).max() <= EPS
    # with exclude_history no returned id is in the row's history
    ids = out["current_token_ids"]
    ex = m.retrieve(b, cat, k, heads=heads, exclude_history=True)
    e_ids, e_scores, _, _ = cat.topk(q, k, exclude_ids=ids)
    assert torch.equal(ex["item_ids"], e_ids) and torch.equal(ex["scores"], e_scores)
    hits_plain = 0
    for i in range(ids.shape[0]):
        hist = set(ids[i].tolist()) - {0}
        got = set(ex["item_ids"][i].tolist()) - {0}
        assert len(got) == k and not got & hist, i
        hits_plain += len(set(res["item_ids"][i].tolist()) & hist)
    assert hits_plain > 0  # the lists without exclusion do hold history items: the exclusion had something to do
    # heads=None is the single-head call it was, and one head is that head's call
    for head in (0, 2):
        q1 = y[:, -1, head].contiguous()
        if q1.dtype not in (torch.float32, torch.bfloat16):
            q1 = q1.float()
        p_ids, p_scores, _, _ = cat.topk(q1, k)
        a = m.retrieve(b, cat, k, head=head)
        assert torch.equal(a["item_ids"], p_ids) and torch.equal(a["scores"], p_scores)
        one = m.retrieve(b, cat, k, heads=[head])
        assert torch.equal(one["item_ids"], p_ids) and torch.equal(one["scores"], p_scores)
    for bad in ([0, 0], [0, len(m._lookahead)], [-1], [], list(range(9))):
        with pytest.raises(ValueError):
            m.retrieve(b, cat, k, heads=bad)


# ------------------------------------------------------------------ 13. script
class ServeHeads(nn.Module):
    def forward(self, q: torch.Tensor, items: torch.Tensor, seen: Optional[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
        scores, rows = torch.ops.lthm.retrieve_topk_group(q, items, 7, True, seen)
        return scores, rows


def test_scripted_op(dev):
    from recommendations_amd import _lib
    from recommendations_amd import kernels as K
    _lib.load_torch_ops()
    assert (str(torch.ops.lthm.retrieve_topk_group.default._schema)
            == "lthm::retrieve_topk_group(Tensor q, Tensor items, int k, bool normalize_q, Tensor? exclude_rows=None) "
               "-> (Tensor scores, Tensor rows)")
    sm = torch.jit.script(ServeHeads())
    assert "lthm::retrieve_topk_group" in str(sm.graph)
    g = torch.Generator().manual_seed(2)
    q = torch.randn(37, 5, 128, generator=g).to(dev)
    items = F.normalize(torch.randn(3001, 128, generator=g), dim=-1).to(torch.bfloat16).to(dev)
    e_scores, e_rows, _, _ = K.retrieve_topk_group(q, items, 7, normalize_q=True)
    scores, rows = sm(q, items, None)
    assert torch.equal(scores, e_scores) and torch.equal(rows, e_rows)
    seen = torch.cat([e_rows[:, :3], torch.randint(-1, 3001, (37, 9), generator=g).to(torch.int32).to(dev)], dim=1).contiguous()
    scores, rows = sm(q, items, seen)
    x_scores, x_rows, _, _ = K.retrieve_topk_group(q, items, 7, normalize_q=True, exclude_rows=seen)
    assert torch.equal(scores, x_scores) and torch.equal(rows, x_rows)
    assert not bool((rows[:, :, None] == e_rows[:, None, :3]).any())
    for bad_q, bad_seen in ((q, seen.long()), (q, seen[:5]), (q[:, 0], None), (q.repeat(1, 2, 1), None)):
        with pytest.raises(RuntimeError):
            torch.ops.lthm.retrieve_topk_group(bad_q, items, 7, True, bad_seen)
