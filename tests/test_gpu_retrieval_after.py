"""Retrieval cursors (lthm_retrieve_topk_after; K.retrieve_topk's and K.retrieve_topk_group's
after_scores / after_rows and deep; ItemCatalogue.topk's after_scores / after_ids;
LTHMModelWrapper.retrieve's after; torch.ops.lthm.retrieve_topk_after) against the checker of
retrieval_after_case.py, which test_retrieval_after_host.py pins on the CPU.

Definition under test: row j with f32 score s_j is eligible iff s_j < after_score or (s_j ==
after_score and j > after_row); a row that is not is scored -inf exactly as an excluded row is (no
slot, no count in rank, target_score the plain dot, tail -1 / -inf).  So a page's last (score,
row) as the next cursor continues the same total order, whatever slab_rows or Q either call used.

Exact cases: integer operands in {-1, 0, 1}, normalize_q=False, so every partial sum is an integer
below 2^8 and scores, rows, rank and target_score must match the checker bit for bit.  The
catalogue is 48 distinct rows repeated at permuted positions (N = 1,500 = 23 tiles + 28 rows, or
N = 700 = 10 tiles + 60 rows), so every score comes in a run of about N / 48 tied rows spread over
the whole catalogue: a run crosses tile and slab boundaries, and a cursor in its middle shows a
wrong > / >= or an off-by-one in the element-to-row mapping.  Q = 70 is two query tiles, one
partial; slab_rows = 64 makes one slab per tile (most hold fewer than k rows), 0 one slab.

Unit-vector case: eps = 1e-5 as in test_gpu_retrieval.py (f32 accumulation of 128 products of
unit vectors errs by at most 128 * 2^-24 <= 7.7e-6; a bf16-representable unit query re-normalises
to itself)."""
from typing import Optional, Tuple

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from lthm_step_case import build_wrapper, load_case
from retrieval_after_case import after_checker

pytestmark = pytest.mark.gpu

EPS = 1e-5
D = 128
Q = 70
INT_MAX = 2 ** 31 - 1
SLABS = [64, 0]
NEG_INF_BITS = np.array([-np.inf], dtype=np.float32).view(np.uint32)[0]
_CACHE = {}


def int_case(N=1500):
    """items [N, 128] bf16 (48 distinct rows, repeated), queries [70, 128] f32 and grouped queries
    [35, 8, 128] f32, all in {-1, 0, 1}; the checker's full order of the plain call (k = N)."""
    key = ("int", N)
    if key not in _CACHE:
        g = torch.Generator().manual_seed(4321 + N)
        base = torch.randint(-1, 2, (48, D), generator=g)
        src = torch.randint(0, 48, (N,), generator=g)
        items = base[src].to(torch.bfloat16)
        q = torch.randint(-1, 2, (Q, D), generator=g).float()
        q3 = torch.randint(-1, 2, (35, 8, D), generator=g).float()
        full = after_checker(q.to(torch.bfloat16), items, N)
        _CACHE[key] = (q, items, q3, full)
    return _CACHE[key]


def targets(n, N):
    trow = ((torch.arange(n) * 7919 + 3) % N).to(torch.int32)
    trow[::5] = -1
    return trow


def run(dev, q, items, k, slab_rows, asc=None, arow=None, tags=None, filt=None, excl=None, trow=None, deep=False,
        normalize_q=False):
    """One call (grouped for a 3-D q); the outputs as numpy arrays (scores as their bits)."""
    from recommendations_amd import kernels as K
    i32 = lambda x: torch.from_numpy(np.asarray(x, dtype=np.int64)).to(torch.int32).contiguous().to(dev)
    call = K.retrieve_topk_group if q.dim() == 3 else K.retrieve_topk
    scores, rows, rank, tscore = call(
        q.contiguous().to(dev), items.to(dev), k, normalize_q=normalize_q, slab_rows=slab_rows,
        exclude_rows=None if excl is None else i32(excl), target_rows=None if trow is None else trow.to(dev),
        tags=None if tags is None else i32(tags), tag_filter=None if filt is None else i32(filt),
        after_scores=None if asc is None else torch.from_numpy(np.asarray(asc, dtype=np.float32)).to(dev),
        after_rows=None if arow is None else i32(arow), deep=deep)
    assert scores.shape == (q.shape[0], k) and rows.shape == (q.shape[0], k)
    out = [scores.cpu().numpy().view(np.uint32), rows.cpu().numpy()]
    if trow is not None:
        out += [rank.cpu().numpy(), tscore.cpu().numpy().view(np.uint32)]
    return out


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def expect_exact(dev, q, items, k, slab_rows, asc, arow, tags=None, filt=None, excl=None, trow=None, deep=False):
    ref = after_checker(q.to(torch.bfloat16), items, k, asc, arow, tags, filt, excl, None if trow is None else trow.numpy())
    _, masked, e_sc, e_rows, e_rank, e_ts = ref
    got = run(dev, q, items, k, slab_rows, asc, arow, tags, filt, excl, trow, deep)
    assert np.array_equal(got[1], e_rows), (slab_rows, k)
    assert np.array_equal(got[0], e_sc.view(np.uint32)), (slab_rows, k)
    if trow is not None:
        assert np.array_equal(got[2], e_rank), slab_rows
        assert np.array_equal(got[3], e_ts.view(np.uint32)), slab_rows  # the plain dot, eligible or not
    return got, ref


def mid_run_cursors(full, n, N, first=30):
    """Query i's cursor is entry first + i of its full order: (score, row) in the middle of a tie
    run.  Returns (asc, arow, pos)."""
    pos = first + np.arange(n)
    asc = full[2][np.arange(n), pos].copy()
    arow = full[3][np.arange(n), pos].astype(np.int64)
    return asc, arow, pos


# ------------------------------------------------------------------ 1. cursors inside tie runs
@pytest.mark.parametrize("slab_rows", SLABS)
def test_cursor_inside_tie_runs(dev, slab_rows):
    q, items, _, full = int_case()
    N = 1500
    asc, arow, pos = mid_run_cursors(full, Q, N)
    # on the checker alone: the cursors sit inside runs that go on behind them, across a tile
    # (= slab at slab_rows 64) boundary
    sc, rows = full[2], full[3]
    inside = crossing = 0
    for i in range(Q):
        p = pos[i]
        if sc[i, p - 1] == sc[i, p] == sc[i, p + 1]:
            inside += 1
            crossing += int(rows[i, p - 1] // 64 != rows[i, p + 1] // 64)
    assert inside >= 60 and crossing >= 40
    trow = targets(Q, N)
    trow[1], trow[2] = int(arow[1]), int(rows[2, 0])  # the cursor row itself and the best row: both ineligible
    got, _ = expect_exact(dev, q, items, 100, slab_rows, asc, arow, trow=trow)
    for i in range(Q):  # the page is the full order's next 100 entries
        assert np.array_equal(got[1][i], rows[i, pos[i] + 1:pos[i] + 101]), i
    # the row term alone: the same scores with after_row at -1, at a row between two members of the
    # run, at N - 1, N and INT_MAX, and at INT_MIN
    kinds = [-1, None, N - 1, N, INT_MAX, -(2 ** 31)]
    arow2 = arow.copy()
    for i in range(Q):
        kind = kinds[i % len(kinds)]
        arow2[i] = arow[i] + 1 if kind is None else kind
    _, ref = expect_exact(dev, q, items, 100, slab_rows, asc, arow2, trow=trow)
    for i in range(Q):
        run_rows = np.nonzero(full[0][i].astype(np.float32) == asc[i])[0]
        head = ref[3][i][ref[2][i] == asc[i]]
        if arow2[i] < 0:
            assert np.array_equal(head, run_rows[:100]), i  # the whole run
        elif arow2[i] >= N - 1:
            assert head.size == 0, i  # none of it


# ------------------------------------------------------------------ 2. +inf is the plain call, -inf and NaN the empty list
@pytest.mark.parametrize("slab_rows", SLABS)
@pytest.mark.parametrize("k", [1, 50, 128])
def test_infinite_cursors(dev, k, slab_rows):
    q, items, q3, _ = int_case()
    N = 1500
    trow = targets(Q, N)
    g = torch.Generator().manual_seed(k)
    arow = torch.randint(-5, N + 5, (Q,), generator=g).numpy()
    plain = run(dev, q, items, k, slab_rows, trow=trow)
    assert same(run(dev, q, items, k, slab_rows, np.full(Q, np.inf), arow, trow=trow), plain)
    for bad in (-np.inf, np.nan):
        got = run(dev, q, items, k, slab_rows, np.full(Q, bad), arow, trow=trow)
        assert (got[1] == -1).all() and (got[0] == NEG_INF_BITS).all()
        assert np.array_equal(got[2], np.where(trow.numpy() >= 0, 0, -1)) and np.array_equal(got[3], plain[3])
    U = 35
    qs = q3[:, :3].contiguous()
    tu = targets(U, N)
    plain = run(dev, qs, items, k, slab_rows, trow=tu)
    assert same(run(dev, qs, items, k, slab_rows, np.full(U, np.inf), arow[:U], trow=tu), plain)
    got = run(dev, qs, items, k, slab_rows, np.full(U, -np.inf), arow[:U], trow=tu)
    assert (got[1] == -1).all() and (got[0] == NEG_INF_BITS).all() and np.array_equal(got[2], np.where(tu.numpy() >= 0, 0, -1))


# ------------------------------------------------------------------ 3. two pages are one list
def test_paging_identity(dev):
    q, items, _, full = int_case()
    whole = run(dev, q, items, 100, 64)
    assert np.array_equal(whole[1], full[3][:, :100])
    page1 = run(dev, q, items, 50, 64)
    assert same([x[:, :50] for x in whole], page1)
    asc, arow = page1[0][:, -1].copy().view(np.float32), page1[1][:, -1]
    assert (full[2][:, 49] == full[2][:, 50]).sum() >= 50  # most cursors sit inside a tie run
    for slab_rows in SLABS:
        page2 = run(dev, q, items, 50, slab_rows, asc, arow)
        assert same([x[:, 50:] for x in whole], page2), slab_rows
        part = run(dev, q[10:20], items, 50, slab_rows, asc[10:20], arow[10:20])  # other queries batched with these or not
        assert same([x[10:20, 50:] for x in whole], part), slab_rows


# ------------------------------------------------------------------ 4. deep lists
@pytest.mark.parametrize("N", [1500, 700])
def test_deep_list_exact(dev, N):
    q, items, q3, full = int_case(N)
    trow = targets(Q, N)
    got = run(dev, q, items, 1024, 64, trow=trow, deep=True)
    n = min(N, 1024)
    assert np.array_equal(got[1][:, :n], full[3][:, :n]) and np.array_equal(got[0][:, :n], full[2][:, :n].view(np.uint32))
    assert (got[1][:, n:] == -1).all() and (got[0][:, n:] == NEG_INF_BITS).all()  # N = 700: the list runs out
    first = run(dev, q, items, 128, 64, trow=trow)
    assert np.array_equal(got[2], first[2]) and np.array_equal(got[3], first[3])  # rank and target_score: the first pass's
    # a caller's cursor is the first pass's; k = 129 is two passes, the second of one row
    asc, arow, pos = mid_run_cursors(full, Q, N)
    got = run(dev, q, items, 129, 0, asc, arow, deep=True)
    for i in range(Q):
        assert np.array_equal(got[1][i], full[3][i, pos[i] + 1:pos[i] + 130]), i
    # grouped
    qs = q3[:, :3].contiguous()
    ref = after_checker(qs.to(torch.bfloat16), items, 300)
    got = run(dev, qs, items, 300, 64, deep=True)
    assert np.array_equal(got[1], ref[3]) and np.array_equal(got[0], ref[2].view(np.uint32))


@pytest.mark.parametrize("N", [1500, 700])
def test_deep_list_unit_vectors(dev, N):
    from recommendations_amd import kernels as K
    nq, k = 40, 1024
    g = torch.Generator().manual_seed(47 + N)
    items = F.normalize(torch.randn(N, D, generator=g), dim=-1).to(torch.bfloat16)
    q = F.normalize(torch.randn(nq, D, generator=g), dim=-1).to(torch.bfloat16).float()
    assert torch.equal(F.normalize(q, dim=-1).to(torch.bfloat16).float(), q)  # the kernel's bf16 operand is q itself
    s = after_checker(q.to(torch.bfloat16), items, 1)[0]
    scores, rows, _, _ = K.retrieve_topk(q.to(dev), items.to(dev), k, normalize_q=True, slab_rows=64, deep=True)
    g_scores, g_rows = scores.cpu().numpy(), rows.cpu().numpy()
    n = min(N, k)
    for i in range(nq):
        r = g_rows[i, :n]
        assert (r >= 0).all() and (r < N).all() and len(set(r.tolist())) == n  # no row twice, also across passes
        assert (g_rows[i, n:] == -1).all() and np.isneginf(g_scores[i, n:]).all()
        sc = g_scores[i, :n]
        assert ((sc[:-1] > sc[1:]) | ((sc[:-1] == sc[1:]) & (r[:-1] < r[1:]))).all()  # strictly descending keys
        assert np.abs(sc.astype(np.float64) - s[i, r]).max() <= EPS
        if n < N:
            kth = np.sort(s[i])[::-1][n - 1]
            assert set(np.nonzero(s[i] > kth + EPS)[0].tolist()) <= set(r.tolist())
            assert (s[i, r] >= kth - EPS).all()


# ------------------------------------------------------------------ 5. composition
@pytest.mark.parametrize("X", [5, 1024])
def test_with_exclusion(dev, X):
    q, items, _, full = int_case()
    N = 1500
    asc, arow, pos = mid_run_cursors(full, Q, N)
    g = torch.Generator().manual_seed(X)
    excl = np.full((Q, X), -1, dtype=np.int64)
    for i in range(Q):
        nxt = full[3][i, pos[i] + 1:pos[i] + 4].tolist()  # the cursor row itself, rows before it, the next three
        lst = [int(arow[i]), int(full[3][i, 0])] + nxt
        if X > 5:
            lst += torch.randperm(N, generator=g)[:900].tolist() + [-1, N, INT_MAX]
        lst = [lst[j] for j in torch.randperm(len(lst), generator=g).tolist()]
        excl[i, :len(lst)] = lst
    trow = targets(Q, N)
    for slab_rows in SLABS:
        got, _ = expect_exact(dev, q, items, 100, slab_rows, asc, arow, excl=excl, trow=trow)
        for i in range(Q):
            assert not set(got[1][i].tolist()) & set(full[3][i, :pos[i] + 4].tolist()), i


@pytest.mark.parametrize("G", [2, 3, 8])
def test_with_groups(dev, G):
    _, items, q3, _ = int_case()
    N, U = 1500, 35
    qs = q3[:, :G].contiguous()
    full = after_checker(qs.to(torch.bfloat16), items, 200)
    asc, arow, pos = mid_run_cursors(full, U, N)
    assert (full[2][np.arange(U), pos] == full[2][np.arange(U), pos + 1]).sum() >= 25
    trow = targets(U, N)
    for slab_rows in SLABS:
        got, _ = expect_exact(dev, qs, items, 100, slab_rows, asc, arow, trow=trow)
        for i in range(U):
            assert np.array_equal(got[1][i], full[3][i, pos[i] + 1:pos[i] + 101]), i


def _tags10(N, seed):
    rng = np.random.default_rng(seed)
    tags = rng.integers(0, 1 << 31, N, dtype=np.int64) & ~np.int64(1)
    tags[rng.random(N) < 0.1] |= 1
    return tags


def test_with_tag_filter(dev):
    q, items, _, _ = int_case()
    N = 1500
    tags = _tags10(N, 5)
    assert 100 < (tags & 1).sum() < 200
    filt = np.tile(np.array([[1, 0, 0]], dtype=np.int64), (Q, 1))
    full = after_checker(q.to(torch.bfloat16), items, 300, None, None, tags, filt)  # -1 behind the eligible rows
    asc, arow, pos = mid_run_cursors(full, Q, N, first=3)  # the filtered order's entry 3 + i
    trow = targets(Q, N)
    for slab_rows in SLABS:
        got, _ = expect_exact(dev, q, items, 100, slab_rows, asc, arow, tags, filt, trow=trow)
        for i in range(Q):
            assert np.array_equal(got[1][i], full[3][i, pos[i] + 1:pos[i] + 101]), i
    assert (got[1][:, -1] == -1).sum() >= 10 and (got[1][:, -1] >= 0).sum() >= 10  # about 150 eligible rows: some pages run out


@pytest.mark.parametrize("G", [3])
def test_all_together(dev, G):
    _, items, q3, _ = int_case()
    N, U = 1500, 35
    qs = q3[:, :G].contiguous()
    tags = _tags10(N, 6) | (np.arange(N) % 2 << 1)
    filt = np.zeros((U, 3), dtype=np.int64)
    filt[0::2] = [0, 0, 1]  # not the marked tenth
    filt[1::2] = [2, 0, 0]  # odd rows
    g = torch.Generator().manual_seed(8)
    excl = np.stack([torch.randperm(N, generator=g)[:64].numpy() for _ in range(U)])
    full = after_checker(qs.to(torch.bfloat16), items, 200, None, None, tags, filt, excl)
    asc, arow, pos = mid_run_cursors(full, U, N)
    trow = targets(U, N)
    for slab_rows in SLABS:
        got, _ = expect_exact(dev, qs, items, 100, slab_rows, asc, arow, tags, filt, excl, trow)
        for i in range(U):
            assert np.array_equal(got[1][i], full[3][i, pos[i] + 1:pos[i] + 101]), i
    got, _ = expect_exact(dev, qs, items, 128, 64, asc, arow, tags, filt, excl, trow)


def test_ineligible_target_is_still_ranked(dev):
    q, items, _, full = int_case()
    N = 1500
    asc, arow, pos = mid_run_cursors(full, Q, N, first=200)
    rows = full[3]
    trow = torch.from_numpy(np.array([rows[i, 120 + i] for i in range(Q)], dtype=np.int32))  # ahead of the cursor
    got, ref = expect_exact(dev, q, items, 10, 64, asc, arow, trow=trow)
    plain = run(dev, q, items, 10, 64, trow=trow)
    assert np.array_equal(got[3], plain[3]) and (got[2] == 0).all() and (plain[2] > 0).all()  # nothing eligible scores above it
    trow = torch.from_numpy(np.array([rows[i, 900 + i] for i in range(Q)], dtype=np.int32))  # behind the cursor
    got, ref = expect_exact(dev, q, items, 10, 0, asc, arow, trow=trow)
    plain = run(dev, q, items, 10, 0, trow=trow)
    assert (got[2] > 0).all() and (got[2] < plain[2]).all() and (plain[2] - got[2] <= pos + 1).all()


# ------------------------------------------------------------------ 6. refusals
def test_refusals(dev):
    from recommendations_amd import kernels as K
    N = 100
    items = torch.zeros((N, D), dtype=torch.bfloat16, device=dev)
    q = torch.zeros((4, D), device=dev)
    q3 = torch.zeros((4, 3, D), device=dev)
    cs = torch.zeros(4, device=dev)
    cr = torch.zeros(4, dtype=torch.int32, device=dev)
    for call, qq in ((K.retrieve_topk, q), (K.retrieve_topk_group, q3)):
        call(qq, items, 5, after_scores=cs, after_rows=cr)
        bad = [dict(after_scores=cs), dict(after_rows=cr), dict(after_scores=cs.double(), after_rows=cr),
               dict(after_scores=cs, after_rows=cr.long()), dict(after_scores=cs[:3], after_rows=cr),
               dict(after_scores=cs, after_rows=torch.zeros(12, dtype=torch.int32, device=dev)),
               dict(after_scores=cs.view(4, 1), after_rows=cr),
               dict(after_scores=torch.zeros(8, device=dev)[::2], after_rows=cr),
               dict(after_scores=cs.cpu(), after_rows=cr), dict(after_scores=cs, after_rows=cr.cpu())]
        for kw in bad:
            with pytest.raises(K.OperandError):
                call(qq, items, 5, **kw)
        with pytest.raises(K.OperandError):
            call(qq, items, 129)  # without deep the cap is the kernel's
        with pytest.raises(K.OperandError):
            call(qq, items, 1025, deep=True)
        assert call(qq, items, 129, deep=True)[1].shape == (4, 129)


# ------------------------------------------------------------------ 7. interface
def test_catalogue_id_cursor(dev):
    from recommendations_amd.models.lthm.sequence.retrieval import ItemCatalogue
    q, items, _, full = int_case(700)
    N = 700
    ids = (torch.arange(N, dtype=torch.int64) * 3 + 5).to(dev)
    cat = ItemCatalogue(ids, items.to(dev))
    qd = q.to(dev)
    whole = cat.topk(qd, 60, normalize_q=False)
    page1 = cat.topk(qd, 30, normalize_q=False)
    page2 = cat.topk(qd, 30, normalize_q=False, after_scores=page1[1][:, -1], after_ids=page1[0][:, -1])
    assert torch.equal(torch.cat([page1[0], page2[0]], 1), whole[0]) and torch.equal(torch.cat([page1[1], page2[1]], 1), whole[1])
    # the cursor's item leaves the catalogue: the next page is the same, from the smaller catalogue
    gone = page1[0][:, -1]
    keep = ~torch.isin(ids, gone)
    small = ItemCatalogue(ids[keep], items.to(dev)[keep])
    assert bool((small.rows_of(gone) == -1).all())
    page2s = small.topk(qd, 30, normalize_q=False, after_scores=page1[1][:, -1], after_ids=gone)
    want = small.topk(qd, 100, normalize_q=False)
    for i in range(Q):  # the small catalogue's own order, from behind (score, id)
        w_ids, w_sc = want[0][i], want[1][i]
        behind = (w_sc < page1[1][i, -1]) | ((w_sc == page1[1][i, -1]) & (w_ids > gone[i]))
        assert torch.equal(page2s[0][i], w_ids[behind][:30]) and torch.equal(page2s[1][i], w_sc[behind][:30]), i
    # an id between two catalogue ids, and k above 128
    mid = cat.topk(qd, 30, normalize_q=False, after_scores=page1[1][:, -1], after_ids=page1[0][:, -1] + 1)
    assert torch.equal(mid[0], page2[0])
    deep = cat.topk(qd, 200, normalize_q=False)
    assert torch.equal(cat.rows_of(deep[0]).cpu(), torch.from_numpy(full[3][:, :200]))
    # an exhausted page's last column ends the paging
    last = cat.topk(qd, 30, normalize_q=False, after_scores=torch.full((Q,), -float("inf"), device=dev),
                    after_ids=torch.zeros(Q, dtype=torch.int64, device=dev))
    assert bool((last[0] == 0).all()) and bool(torch.isneginf(last[1]).all())


def test_wrapper_retrieve_pages(dev):
    from recommendations_amd.models.lthm.sequence.retrieval import build_catalogue
    fx, params, _, batch = load_case("lthm_step_a")
    m = build_wrapper(fx, params, dev).eval()
    b = {k: v.to(dev) for k, v in batch.items()}
    ids = batch["product_ids"].reshape(-1)
    g = torch.Generator().manual_seed(5)
    extra = torch.randint(1, 2 ** 62, (300,), generator=g)
    all_ids = torch.cat([extra, ids[ids != 0]])
    tg = (torch.unique(all_ids) % 4).to(torch.int32)
    cat = build_catalogue(m, torch.unique(all_ids), chunk=128, tags=tg)
    k = 20
    for kw in (dict(), dict(exclude_history=True, heads=[0, 2], tag_none=1)):
        whole = m.retrieve(b, cat, 2 * k, **kw)
        page1 = m.retrieve(b, cat, k, **kw)
        page2 = m.retrieve(b, cat, k, after=page1, **kw)
        page2t = m.retrieve(b, cat, k, after=(page1["scores"][:, -1], page1["item_ids"][:, -1]), **kw)
        assert bool((page2["item_ids"] != 0).all())
        for key in ("item_ids", "scores"):
            assert torch.equal(torch.cat([page1[key], page2[key]], 1), whole[key]), (key, kw)
            assert torch.equal(page2[key], page2t[key])
    deep = m.retrieve(b, cat, 150)
    assert deep["item_ids"].shape[1] == 150 and torch.equal(deep["item_ids"][:, :2 * k], m.retrieve(b, cat, 2 * k)["item_ids"])
    for i in range(deep["item_ids"].shape[0]):
        assert len(set(deep["item_ids"][i].tolist())) == 150
    with pytest.raises(ValueError):
        m.retrieve(b, cat, k, after=(page1["scores"], page1["item_ids"]))


class ServeNext(nn.Module):
    def forward(self, q: torch.Tensor, items: torch.Tensor, seen: Optional[torch.Tensor], tags: Optional[torch.Tensor],
                filt: Optional[torch.Tensor], after_scores: torch.Tensor,
                after_rows: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        scores, rows = torch.ops.lthm.retrieve_topk_after(q, items, 7, True, seen, tags, filt, after_scores, after_rows)
        return scores, rows


def test_scripted_op(dev):
    from recommendations_amd import _lib
    from recommendations_amd import kernels as K
    _lib.load_torch_ops()
    assert (str(torch.ops.lthm.retrieve_topk_after.default._schema)
            == "lthm::retrieve_topk_after(Tensor q, Tensor items, int k, bool normalize_q, Tensor? exclude_rows, "
               "Tensor? tags, Tensor? tag_filter, Tensor after_scores, Tensor after_rows) -> (Tensor scores, Tensor rows)")
    sm = torch.jit.script(ServeNext())
    assert "lthm::retrieve_topk_after" in str(sm.graph)
    g = torch.Generator().manual_seed(2)
    q3 = torch.randn(37, 5, 128, generator=g).to(dev)
    q2 = q3[:, 0].contiguous()
    items = F.normalize(torch.randn(1501, 128, generator=g), dim=-1).to(torch.bfloat16).to(dev)
    tags = torch.randint(0, 4, (1501,), generator=g).to(torch.int32).to(dev)
    filt = torch.tensor([[0, 0, 1]], dtype=torch.int32).repeat(37, 1).to(dev)
    seen = torch.randint(-1, 1501, (37, 12), generator=g).to(torch.int32).to(dev)
    for q, eager in ((q2, K.retrieve_topk), (q3, K.retrieve_topk_group)):
        for x in (None, seen):
            for tg, fl in ((None, None), (tags, filt)):
                p_scores, p_rows, _, _ = eager(q, items, 7, normalize_q=True, exclude_rows=x, tags=tg, tag_filter=fl)
                cs, cr = p_scores[:, -1].contiguous(), p_rows[:, -1].contiguous()
                e_scores, e_rows, _, _ = eager(q, items, 7, normalize_q=True, exclude_rows=x, tags=tg, tag_filter=fl,
                                               after_scores=cs, after_rows=cr)
                scores, rows = sm(q, items, x, tg, fl, cs, cr)
                assert torch.equal(scores, e_scores) and torch.equal(rows, e_rows)
                both = eager(q, items, 14, normalize_q=True, exclude_rows=x, tags=tg, tag_filter=fl)
                assert torch.equal(torch.cat([p_rows, rows], 1), both[1]) and torch.equal(torch.cat([p_scores, scores], 1), both[0])
    cs, cr = torch.zeros(37, device=dev), torch.zeros(37, dtype=torch.int32, device=dev)
    for bad in (dict(cs=cs.double()), dict(cr=cr.long()), dict(cs=cs[:5]), dict(cr=cr[:5]), dict(cs=cs.cpu()),
                dict(tags=tags), dict(filt=filt), dict(q=q2[0])):
        a = dict(q=q2, tags=None, filt=None, cs=cs, cr=cr)
        a.update(bad)
        with pytest.raises(RuntimeError):
            torch.ops.lthm.retrieve_topk_after(a["q"], items, 7, True, None, a["tags"], a["filt"], a["cs"], a["cr"])
