"""Single-scan deep lists (lthm_retrieve_topk_deep; K.retrieve_topk's and K.retrieve_topk_group's
deep=True; torch.ops.lthm.retrieve_topk_deep): 129 <= k <= 1,024 rows per query from one scan of
the catalogue.

Definition under test: the four outputs are, bit for bit, those of the paged path (deep="paged":
ceil(k / 128) calls of the k <= 128 kernel, each behind the last column of the one before), and
both are held to the fp64 checkers of retrieval_after_case.py / retrieval_bias_case.py directly.

Exact cases: integer operands in {-1, 0, 1}, normalize_q=False, biases in multiples of 0.5 and
small integer weights, so every f32 in the kernel is exact and the checker must be met bit for
bit.  The catalogue is 48 distinct rows repeated at random positions, so every score comes in a
tie run spread over the whole catalogue and every rank of every list sits inside a run.  N = 3,000
is 46 tiles + 56 rows; Q = 70 is two query tiles, the second partial; slab_rows = 64 makes one slab
per tile (none holds k rows: the merge does the selecting), 0 one slab (the in-slab sort does).

Unit-vector case: eps = 1e-5 as in test_gpu_retrieval.py (f32 accumulation of 128 products of unit
vectors errs by at most 128 * 2^-24 <= 7.7e-6; a bf16-representable unit query re-normalises to
itself).

The prune cases use one slab of N = 8,192 rows, four times the kernel's 2,048 key slots per
query, so a full buffer is sorted and cut back to k several times over."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from retrieval_after_case import after_checker
from retrieval_bias_case import bias_checker

pytestmark = pytest.mark.gpu

EPS = 1e-5
D = 128
N = 3000
Q = 70
KS = [129, 300, 1000, 1024]
SLABS = [64, 0]
_CACHE = {}


def int_case():
    """items [N, 128] bf16, q [70, 128] f32, q3 [70, 3, 128] f32, and the pieces of the full
    composition: exclusion lists, tags and filters, bias and weights, targets."""
    if "int" not in _CACHE:
        g = torch.Generator().manual_seed(9091)
        base = torch.randint(-1, 2, (48, D), generator=g)
        items = base[torch.randint(0, 48, (N,), generator=g)].to(torch.bfloat16)
        q = torch.randint(-1, 2, (Q, D), generator=g).float()
        q3 = torch.randint(-1, 2, (Q, 3, D), generator=g).float()
        excl = torch.randint(-2, N + 2, (Q, 37), generator=g).to(torch.int32)
        tags = torch.randint(0, 8, (N,), generator=g).to(torch.int32)
        filt = torch.tensor([[1, 0, 0], [0, 6, 0], [0, 0, 4], [0, 0, 0], [1, 2, 4]], dtype=torch.int32).repeat(Q // 5, 1)
        bias = (torch.randint(-4, 5, (N,), generator=g).float() * 0.5)
        bw = torch.randint(-1, 3, (Q,), generator=g).float()
        trow = ((torch.arange(Q) * 7919 + 3) % N).to(torch.int32)
        trow[::5] = -1
        _CACHE["int"] = dict(items=items, q=q, q3=q3, excl=excl, tags=tags, filt=filt.contiguous(), bias=bias, bw=bw,
                             trow=trow)
    return _CACHE["int"]


def cursors(c):
    """A caller's cursor per user inside a tie run of the composed order: entry 30 + u of the list
    without a cursor, from the checker (computed once)."""
    if "cur" not in _CACHE:
        ref = bias_checker(c["q3"].to(torch.bfloat16), c["items"], 30 + Q, c["bias"].numpy(), c["bw"].numpy(),
                           tags=c["tags"].numpy(), filt=c["filt"].numpy(), excl=c["excl"].numpy())
        pos = 30 + np.arange(Q)
        _CACHE["cur"] = (torch.from_numpy(ref["scores"][np.arange(Q), pos].copy()),
                         torch.from_numpy(ref["rows"][np.arange(Q), pos].copy()))
    return _CACHE["cur"]


def call(dev, q, items, k, deep, slab_rows=0, normalize_q=False, **kw):
    """One call (grouped for a 3-D q) -> [scores as int32 bits, rows, rank, target_score bits] on
    the CPU, None where the call returns None."""
    from recommendations_amd import kernels as K
    fn = K.retrieve_topk_group if q.dim() == 3 else K.retrieve_topk
    kw = {name: (v.to(dev) if isinstance(v, torch.Tensor) else v) for name, v in kw.items()}
    out = fn(q.contiguous().to(dev), items.to(dev), k, normalize_q=normalize_q, slab_rows=slab_rows, deep=deep, **kw)
    assert out[0].shape == (q.shape[0], k) and out[1].shape == (q.shape[0], k)
    bits = lambda t: None if t is None else t.cpu().view(torch.int32)
    return [bits(out[0]), out[1].cpu(), None if out[2] is None else out[2].cpu(), bits(out[3])]


def equal(a, b):
    return all((x is None and y is None) or (x is not None and y is not None and torch.equal(x, y)) for x, y in zip(a, b))


def variant(name):
    c = int_case()
    if name == "plain":
        return c["q"], {}
    if name == "targets":
        return c["q"], dict(target_rows=c["trow"])
    cs, cr = cursors(c)
    return c["q3"], dict(target_rows=c["trow"], exclude_rows=c["excl"], tags=c["tags"], tag_filter=c["filt"],
                         after_scores=cs, after_rows=cr, bias=c["bias"], bias_weight=c["bw"])


def against_checker(got, ref):
    """got from call(); ref a bias_checker dict: bit for bit."""
    assert torch.equal(got[1], torch.from_numpy(ref["rows"]))
    assert torch.equal(got[0], torch.from_numpy(ref["scores"]).view(torch.int32))
    if ref["rank"] is not None:
        assert torch.equal(got[2], torch.from_numpy(ref["rank"]))
        assert torch.equal(got[3], torch.from_numpy(ref["tscore"]).view(torch.int32))


# ------------------------------------------------------------------ 1. the paged path, bit for bit
@pytest.mark.parametrize("slab_rows", SLABS)
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", ["plain", "targets", "all"])
def test_equals_the_paged_path(dev, name, k, slab_rows):
    q, kw = variant(name)
    items = int_case()["items"]
    scan = call(dev, q, items, k, True, slab_rows, **kw)
    paged = call(dev, q, items, k, "paged", slab_rows, **kw)
    assert equal(scan, paged)
    assert (scan[2] is not None) == (name != "plain")


# ------------------------------------------------------------------ 2. the fp64 checker, at k = 1,024
@pytest.mark.parametrize("slab_rows", SLABS)
def test_checker_exact(dev, slab_rows):
    c = int_case()
    k = 1024
    if "ref_plain" not in _CACHE:
        _CACHE["ref_plain"] = bias_checker(c["q"].to(torch.bfloat16), c["items"], k, trow=c["trow"].numpy())
        cs, cr = cursors(c)
        _CACHE["ref_all"] = bias_checker(c["q3"].to(torch.bfloat16), c["items"], k, c["bias"].numpy(), c["bw"].numpy(),
                                         cs.numpy(), cr.numpy(), c["tags"].numpy(), c["filt"].numpy(), c["excl"].numpy(),
                                         c["trow"].numpy())
    q, kw = variant("targets")
    against_checker(call(dev, q, c["items"], k, True, slab_rows, **kw), _CACHE["ref_plain"])
    q, kw = variant("all")
    against_checker(call(dev, q, c["items"], k, True, slab_rows, **kw), _CACHE["ref_all"])
    # the composed lists are not all full: some filters leave fewer than k rows
    n_el = (_CACHE["ref_all"]["rows"] >= 0).sum(axis=1)
    assert n_el.min() < k and n_el.max() == k


def test_checker_unit_vectors(dev):
    nq, k = 40, 1024
    g = torch.Generator().manual_seed(4711)
    items = F.normalize(torch.randn(N, D, generator=g), dim=-1).to(torch.bfloat16)
    q = F.normalize(torch.randn(nq, D, generator=g), dim=-1).to(torch.bfloat16).float()
    assert torch.equal(F.normalize(q, dim=-1).to(torch.bfloat16).float(), q)  # the kernel's bf16 operand is q itself
    s = after_checker(q.to(torch.bfloat16), items, 1)[0]
    for slab_rows in SLABS:
        got = call(dev, q, items, k, True, slab_rows, normalize_q=True)
        g_scores, g_rows = got[0].view(torch.float32).numpy(), got[1].numpy()
        for i in range(nq):
            r = g_rows[i]
            assert (r >= 0).all() and (r < N).all() and len(set(r.tolist())) == k
            sc = g_scores[i]
            assert ((sc[:-1] > sc[1:]) | ((sc[:-1] == sc[1:]) & (r[:-1] < r[1:]))).all()  # strictly descending keys
            assert np.abs(sc.astype(np.float64) - s[i, r]).max() <= EPS
            kth = np.sort(s[i])[::-1][k - 1]
            assert set(np.nonzero(s[i] > kth + EPS)[0].tolist()) <= set(r.tolist())
            assert (s[i, r] >= kth - EPS).all()


# ------------------------------------------------------------------ 3. the in-slab prune, worst case
def prune_case(kind):
    n = 8192
    g = torch.Generator().manual_seed(77)
    if kind == "ascending":
        # row j = 64 hi + lo holds (hi, lo); query i holds c_i (64, 1): the score c_i j is exact and
        # strictly ascending in j for c_i > 0, so every row passes the threshold of the rows before
        j = torch.arange(n)
        items = torch.zeros(n, D)
        items[:, 0], items[:, 1] = j // 64, j % 64
        c = torch.tensor([1., 2., 3., 4., 5., 7., 8., -1.])
        q = torch.zeros(8, D)
        q[:, 0], q[:, 1] = 64 * c, c
    elif kind == "equal":
        items = torch.randint(-1, 2, (1, D), generator=g).float().repeat(n, 1)  # one tie run of 8,192
        q = torch.randint(-1, 2, (8, D), generator=g).float()
    else:
        items = torch.randint(-1, 2, (n, D), generator=g).float()
        q = torch.randint(-1, 2, (8, D), generator=g).float()
    return q, items.to(torch.bfloat16)


@pytest.mark.parametrize("k", [129, 1024])
@pytest.mark.parametrize("kind", ["ascending", "equal", "random"])
def test_prune_worst_case(dev, kind, k):
    q, items = prune_case(kind)
    assert items.float().abs().max() <= 256  # exact in bf16
    trow = torch.tensor([0, 8191, -1, 4000, 1, 2, 3, 4], dtype=torch.int32)
    _, _, e_sc, e_rows, e_rank, e_ts = after_checker(q.to(torch.bfloat16), items, k, trow=trow.numpy())
    got = call(dev, q, items, k, True, 8192, target_rows=trow)
    assert torch.equal(got[1], torch.from_numpy(e_rows))
    assert torch.equal(got[0], torch.from_numpy(e_sc).view(torch.int32))
    assert torch.equal(got[2], torch.from_numpy(e_rank)) and torch.equal(got[3], torch.from_numpy(e_ts).view(torch.int32))
    if kind == "ascending":
        assert got[1][0].tolist() == list(range(8191, 8191 - k, -1)) and got[1][7].tolist() == list(range(k))
    if kind == "equal":
        assert (got[1] == torch.arange(k, dtype=torch.int32)).all()


# ------------------------------------------------------------------ 4. short catalogues, exhausted lists
@pytest.mark.parametrize("n", [1, 63, 130])
def test_short_catalogue(dev, n):
    c = int_case()
    items = c["items"][:n]
    ref = bias_checker(c["q"].to(torch.bfloat16), items, 1024)
    for slab_rows in SLABS:
        got = call(dev, c["q"], items, 1024, True, slab_rows)
        against_checker(got, ref)
        assert (got[1][:, n:] == -1).all() and torch.isneginf(got[0][:, n:].view(torch.float32)).all()
        assert (got[1][:, :n] >= 0).all()


@pytest.mark.parametrize("slab_rows", SLABS)
def test_fewer_than_k_eligible(dev, slab_rows):
    c = int_case()
    q, items, trow = c["q"], c["items"], c["trow"]
    # a cursor that admits nothing
    got = call(dev, q, items, 1024, True, slab_rows, target_rows=trow, after_scores=torch.full((Q,), float("-inf")),
               after_rows=torch.full((Q,), -1, dtype=torch.int32))
    assert (got[1] == -1).all() and torch.isneginf(got[0].view(torch.float32)).all()
    assert torch.equal(got[2], torch.where(trow >= 0, 0, -1).to(torch.int32))
    # a tag filter that admits 200 rows
    tags = torch.zeros(N, dtype=torch.int32)
    tags[torch.randperm(N, generator=torch.Generator().manual_seed(5))[:200]] = 1
    filt = torch.tensor([[1, 0, 0]], dtype=torch.int32).repeat(Q, 1).contiguous()
    ref = bias_checker(q.to(torch.bfloat16), items, 1024, tags=tags.numpy(), filt=filt.numpy(), trow=trow.numpy())
    got = call(dev, q, items, 1024, True, slab_rows, target_rows=trow, tags=tags, tag_filter=filt)
    against_checker(got, ref)
    assert (got[1][:, :200] >= 0).all() and (got[1][:, 200:] == -1).all()
    assert (tags[got[1][:, :200].long()] == 1).all()
    assert got[2].max() < 200  # eligible rows only


# ------------------------------------------------------------------ 5. independence of the cut and of Q
@pytest.mark.parametrize("name", ["targets", "all"])
def test_independent_of_the_cut(dev, name):
    q, kw = variant(name)
    items = int_case()["items"]
    first = call(dev, q, items, 1000, True, 64, **kw)
    for slab_rows in (128, 1024, 0):
        assert equal(call(dev, q, items, 1000, True, slab_rows, **kw), first), slab_rows


def test_independent_of_q(dev):
    c = int_case()
    g = torch.Generator().manual_seed(31)
    big = torch.randint(-1, 2, (200, D), generator=g).float()
    big[100:100 + Q] = c["q"]
    trow = torch.full((200,), 17, dtype=torch.int32)
    trow[100:100 + Q] = c["trow"]
    small = call(dev, c["q"], c["items"], 1000, True, 0, target_rows=c["trow"])
    for slab_rows in (0, 128):
        got = call(dev, big, c["items"], 1000, True, slab_rows, target_rows=trow)
        assert equal([t[100:100 + Q] for t in got], small)


# ------------------------------------------------------------------ 6. paging on top of a deep list
def test_paging_on_a_deep_list(dev):
    c = int_case()
    whole = call(dev, c["q"], c["items"], 1024, True)
    head = call(dev, c["q"], c["items"], 600, True)
    cs = head[0][:, -1].view(torch.float32).contiguous()
    cr = head[1][:, -1].contiguous()
    tail = call(dev, c["q"], c["items"], 424, True, after_scores=cs, after_rows=cr)
    assert torch.equal(torch.cat([head[0], tail[0]], dim=1), whole[0])
    assert torch.equal(torch.cat([head[1], tail[1]], dim=1), whole[1])


# ------------------------------------------------------------------ 7. the C ABI through ctypes
def test_c_abi(dev):
    from recommendations_amd import _lib
    lib = _lib.load()
    c = int_case()
    items, q = c["items"].to(dev), c["q"].to(dev)
    bias, trow = c["bias"].to(dev), c["trow"].to(dev)
    cs = torch.full((Q,), float("inf"), device=dev)
    cr = torch.zeros(Q, dtype=torch.int32, device=dev)

    def desc(k, ws):
        out = [torch.full((Q, k), 7.0, device=dev), torch.full((Q, k), 7, dtype=torch.int32, device=dev),
               torch.full((Q,), 7, dtype=torch.int32, device=dev), torch.full((Q,), 7.0, device=dev)]
        d = _lib.STRUCTS["lthm_retrieve_desc"]()
        d.items, d.q, d.target_row = items.data_ptr(), q.data_ptr(), trow.data_ptr()
        d.scores, d.rows, d.rank, d.target_score = (t.data_ptr() for t in out)
        d.workspace, d.ws_bytes = ws.data_ptr(), ws.numel()
        d.Q, d.N, d.k, d.q_dtype, d.normalize_q, d.slab_rows = Q, N, k, _lib.F32, 0, 0
        return d, out

    b = _lib.STRUCTS["lthm_retrieve_bias"]()
    b.bias, b.weight = bias.data_ptr(), None
    cur = _lib.STRUCTS["lthm_retrieve_cursor"]()
    cur.after_score, cur.after_row = cs.data_ptr(), cr.data_ptr()
    stream = torch.cuda.current_stream(dev).cuda_stream
    args = lambda d, cc: (ctypes.addressof(d), None, None, None, ctypes.addressof(cc), ctypes.addressof(b), stream)

    # k = 100: the entry is lthm_retrieve_topk_bias
    need = lib.lthm_retrieve_deep_ws_bytes(Q, 1, N, 100, 0, 0)
    assert need == lib.lthm_retrieve_ws_bytes(Q, N, 100, 0)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    d1, o1 = desc(100, ws)
    assert lib.lthm_retrieve_topk_deep(*args(d1, cur)) == 0
    torch.cuda.synchronize()
    d2, o2 = desc(100, ws)
    assert lib.lthm_retrieve_topk_bias(*args(d2, cur)) == 0
    torch.cuda.synchronize()
    for x, y in zip(o1, o2):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))

    # refusals: the error code, and nothing launched (the outputs keep their fill)
    need = lib.lthm_retrieve_deep_ws_bytes(Q, 1, N, 1024, 0, 0)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    bad = _lib.STRUCTS["lthm_retrieve_cursor"]()
    bad.after_score, bad.after_row = cs.data_ptr(), cr.data_ptr() + 2
    for k, nbytes, cc in ((1024, need - 1, cur), (1025, need, cur), (1024, need, bad)):
        d, out = desc(min(k, 1024), ws)
        d.k, d.ws_bytes = k, nbytes
        assert lib.lthm_retrieve_topk_deep(*args(d, cc)) != 0
        torch.cuda.synchronize()
        assert all((t == 7).all() for t in out)
    # and the good call at k = 1,024 equals the Python path
    d, out = desc(1024, ws)
    assert lib.lthm_retrieve_topk_deep(*args(d, cur)) == 0
    torch.cuda.synchronize()
    ref = call(dev, c["q"], c["items"], 1024, True, target_rows=c["trow"], bias=c["bias"])
    assert equal([out[0].cpu().view(torch.int32), out[1].cpu(), out[2].cpu(), out[3].cpu().view(torch.int32)], ref)


# ------------------------------------------------------------------ 8. the scripted op
def test_scripted_op(dev):
    from typing import Optional, Tuple
    from recommendations_amd import _lib
    _lib.load_torch_ops()

    def f(q: torch.Tensor, items: torch.Tensor, k: int, excl: Optional[torch.Tensor], tags: Optional[torch.Tensor],
          filt: Optional[torch.Tensor], cs: Optional[torch.Tensor], cr: Optional[torch.Tensor],
          bias: Optional[torch.Tensor], bw: Optional[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
        return torch.ops.lthm.retrieve_topk_deep(q, items, k, False, excl, tags, filt, cs, cr, bias, bw)

    sf = torch.jit.script(f)
    assert "lthm::retrieve_topk_deep" in str(sf.graph)
    c = int_case()
    items = c["items"].to(dev)
    s, r = sf(c["q"].to(dev), items, 300, None, None, None, None, None, None, None)
    ref = call(dev, c["q"], c["items"], 300, True)
    assert torch.equal(s.cpu().view(torch.int32), ref[0]) and torch.equal(r.cpu(), ref[1])
    q3, kw = variant("all")
    s, r = sf(q3.to(dev), items, 300, kw["exclude_rows"].to(dev), kw["tags"].to(dev), kw["tag_filter"].to(dev),
              kw["after_scores"].to(dev), kw["after_rows"].to(dev), kw["bias"].to(dev), kw["bias_weight"].to(dev))
    ref = call(dev, q3, c["items"], 300, True, **{n: v for n, v in kw.items() if n != "target_rows"})
    assert torch.equal(s.cpu().view(torch.int32), ref[0]) and torch.equal(r.cpu(), ref[1])
    s, r = sf(c["q"].to(dev), items, 100, None, None, None, None, None, None, None)  # k <= 128: the paged kernels
    ref = call(dev, c["q"], c["items"], 100, False)
    assert torch.equal(s.cpu().view(torch.int32), ref[0]) and torch.equal(r.cpu(), ref[1])
    with pytest.raises(RuntimeError):
        sf(c["q"].to(dev), items, 1025, None, None, None, None, None, None, None)
