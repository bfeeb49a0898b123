"""The exact scan's one launch path (csrc/retrieve.hip, retr_scan) over the whole option lattice, at
the smallest shapes that reach every branch: exclusion x tags x cursor x prior x given target scores
x G in {1, 3} x k in {10, 200}, 128 calls through K.retrieve_topk / K.retrieve_topk_group, each held
bit for bit to the checker of retrieval_bias_case.py.  Then the eight C entry points against
lthm_retrieve_topk_deep, and the KernelTimer's record of every call.

The inputs follow int_case of test_gpu_retrieval_bias.py: items and queries in {-1, 0, 1}, biases in
multiples of 0.5, weights from {0, 0.5, 1, 2, -1}, so that every score is exact in f32 and a list is
a matter of selection alone.  Q = 70 is two query tiles, the second partial; G = 3 is four slots per
user, one padded; slab_rows = 64 cuts N = 300 into five slabs, the last partial."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from retrieval_bias_case import bias_checker

pytestmark = pytest.mark.gpu

D, Q, G, N, X, SLAB = 128, 70, 3, 300, 5, 64
KS = (10, 200)
WEIGHTS = np.array([0.0, 0.5, 1.0, 2.0, -1.0], dtype=np.float32)
_CACHE = {}


def case():
    if "case" not in _CACHE:
        g = torch.Generator().manual_seed(4217)
        rng = np.random.default_rng(4217)
        c = dict(items=torch.randint(-1, 2, (N, D), generator=g).to(torch.bfloat16),
                 q1=torch.randint(-1, 2, (Q, D), generator=g).float(),
                 q3=torch.randint(-1, 2, (Q, G, D), generator=g).float(),
                 bias=(torch.randint(-16, 17, (N,), generator=g).float() * 0.5).numpy(),
                 w=WEIGHTS[np.arange(Q) % 5],
                 tags=rng.integers(0, 8, N, dtype=np.int64))
        filt = np.zeros((Q, 3), dtype=np.int64)  # (all, any, none) over three bits, by turns
        filt[0::3] = [1, 0, 0]
        filt[1::3] = [0, 6, 0]
        filt[2::3] = [0, 0, 4]
        trow = ((torch.arange(Q) * 7919 + 3) % N).to(torch.int32)
        trow[::5] = -1
        excl = rng.integers(0, N, (Q, X), dtype=np.int64)
        excl[:, 0] = np.where(trow.numpy() >= 0, trow.numpy(), excl[:, 0])  # a target on its own list
        excl[:, 1] = -1  # a pad
        tsin = (rng.integers(-40, 41, Q) * 0.25).astype(np.float32)  # the caller's target scores: any f32
        tsin[7] = np.nan
        c.update(filt=filt, trow=trow, excl=excl, tsin=tsin)
        _CACHE["case"] = c
    return _CACHE["case"]


def reference(grouped, x, t, c, b):
    """The checker's k = 200 answer for one point of the lattice (k = 10 is its first columns), with
    the cursor that the point uses: user i's is entry 20 + i of the (G, prior) order without it."""
    key = (grouped, x, t, c, b)
    if key not in _CACHE:
        cs = case()
        qbf = (cs["q3"] if grouped else cs["q1"]).to(torch.bfloat16)
        bias, w = (cs["bias"], cs["w"]) if b else (None, None)
        asc = arow = None
        if c:
            if ("full", grouped, b) not in _CACHE:
                _CACHE["full", grouped, b] = bias_checker(qbf, cs["items"], 20 + Q, bias, w)
            full, pos = _CACHE["full", grouped, b], 20 + np.arange(Q)
            asc, arow = full["scores"][np.arange(Q), pos].copy(), full["rows"][np.arange(Q), pos].astype(np.int64)
        ref = bias_checker(qbf, cs["items"], max(KS), bias, w, asc, arow, cs["tags"] if t else None,
                           cs["filt"] if t else None, cs["excl"] if x else None, cs["trow"].numpy())
        ref["asc"], ref["arow"] = asc, arow
        # rank against given scores: the entries strictly above, the target's own row left out
        tr, ts = cs["trow"].numpy(), cs["tsin"]
        ref["rank_given"] = np.array(
            [-1 if np.isnan(ts[u]) else
             int(((np.delete(ref["masked"][u], tr[u]) if 0 <= tr[u] < N else ref["masked"][u]) > ts[u]).sum())
             for u in range(Q)], dtype=np.int32)
        _CACHE[key] = ref
    return _CACHE[key]


def on_device(dev):
    if "dev" not in _CACHE:
        cs = case()
        i32 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.int64)).to(torch.int32).contiguous().to(dev)
        f32 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32)).contiguous().to(dev)
        _CACHE["dev"] = dict(items=cs["items"].to(dev), q1=cs["q1"].to(dev), q3=cs["q3"].contiguous().to(dev),
                             bias=f32(cs["bias"]), w=f32(cs["w"]), tags=i32(cs["tags"]), filt=i32(cs["filt"]),
                             trow=cs["trow"].to(dev), excl=i32(cs["excl"]), tsin=f32(cs["tsin"]))
    return _CACHE["dev"]


def kwargs(dv, ref, x, t, c, b, ts):
    """The keyword arguments of one point of the lattice, on the device"""
    f32 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32)).to(dv["items"].device)
    i32 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.int64)).to(torch.int32).to(dv["items"].device)
    return dict(normalize_q=False, slab_rows=SLAB, target_rows=dv["trow"], deep=True,
                exclude_rows=dv["excl"] if x else None, tags=dv["tags"] if t else None,
                tag_filter=dv["filt"] if t else None, after_scores=f32(ref["asc"]) if c else None,
                after_rows=i32(ref["arow"]) if c else None, bias=dv["bias"] if b else None,
                bias_weight=dv["w"] if b else None, target_scores=dv["tsin"] if ts else None)


@pytest.mark.parametrize("grouped", [False, True], ids=["G1", "G3"])
@pytest.mark.parametrize("x,t,c,b", list(itertools.product([False, True], repeat=4)))
def test_lattice(dev, x, t, c, b, grouped):
    from recommendations_amd import kernels as K
    dv, ref = on_device(dev), reference(grouped, x, t, c, b)
    fn, q = (K.retrieve_topk_group, dv["q3"]) if grouped else (K.retrieve_topk, dv["q1"])
    for ts, k in itertools.product([False, True], KS):
        scores, rows, rank, tscore = fn(q, dv["items"], k, **kwargs(dv, ref, x, t, c, b, ts))
        at = (ts, k)
        assert np.array_equal(rows.cpu().numpy(), ref["rows"][:, :k]), at
        assert np.array_equal(scores.cpu().numpy().view(np.uint32), ref["scores"][:, :k].view(np.uint32)), at
        if ts:
            assert tscore is dv["tsin"], at  # the tensor given
            assert np.array_equal(rank.cpu().numpy(), ref["rank_given"]), at
        else:
            assert np.array_equal(tscore.cpu().numpy().view(np.uint32), ref["tscore"].view(np.uint32)), at
            assert np.array_equal(rank.cpu().numpy(), ref["rank"]), at


def test_the_lattice_reaches_its_branches():
    """On the checker alone: the masks bite, lists run short of k = 200, a given score changes ranks."""
    cs = case()
    plain, every = reference(False, False, False, False, False), reference(True, True, True, True, True)
    assert (plain["rows"] >= 0).all() and (every["rows"][:, -1] == -1).any() and (every["rows"][:, 9] >= 0).all()
    assert not np.array_equal(every["rows"][:, :10], reference(True, True, True, True, False)["rows"][:, :10])
    assert not np.array_equal(every["rows"][:, :10], reference(True, True, True, False, True)["rows"][:, :10])
    assert not np.array_equal(every["rows"][:, :10], reference(True, True, False, True, True)["rows"][:, :10])
    assert not np.array_equal(every["rank"], reference(True, False, True, True, True)["rank"])
    assert (every["rank_given"] == -1).sum() == 1 and (every["rank"] == -1).sum() == Q // 5
    assert (every["rank_given"] != every["rank"]).sum() > Q // 2
    assert (cs["trow"].numpy() == -1).sum() == Q // 5


# ------------------------------------------------------------------ the C entry points
ENTRIES = [("lthm_retrieve_topk", ""), ("lthm_retrieve_topk_excl", "x"), ("lthm_retrieve_topk_group", "xg"),
           ("lthm_retrieve_topk_tags", "xgt"), ("lthm_retrieve_topk_after", "xgtc"),
           ("lthm_retrieve_topk_bias", "xgtcb"), ("lthm_retrieve_topk_deep", "xgtcb"),
           ("lthm_retrieve_topk_shard", "xgtcbs")]


def raw_call(dev, name, has, present, k, tsin=None):
    """One call of a C entry point that takes the parts `has`, with those of `present` filled in and
    the others NULL, at the lattice's shape with every target valid; the four outputs as bits."""
    from recommendations_amd import _lib
    from recommendations_amd._lib import ptr, stream
    lib, S = _lib.load(), _lib.STRUCTS
    dv = on_device(dev)
    ref = reference("g" in present, "x" in present, "t" in present, True, "b" in present)  # for its cursors
    q = dv["q3"] if "g" in present else dv["q1"]
    trow = (torch.arange(Q, dtype=torch.int32) * 13 % N).to(dev)
    keep = [q, trow]  # what the descriptors point at
    scores = torch.empty((Q, k), dtype=torch.float32, device=dev)
    rows = torch.empty((Q, k), dtype=torch.int32, device=dev)
    rank = torch.empty(Q, dtype=torch.int32, device=dev)
    tscore = torch.empty(Q, dtype=torch.float32, device=dev)
    need = lib.lthm_retrieve_deep_ws_bytes(Q, G if "g" in present else 1, N, k, SLAB, X if "x" in present else 0)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    d = S["lthm_retrieve_desc"]()
    d.items, d.q, d.target_row = ptr(dv["items"]), ptr(q), ptr(trow)
    d.scores, d.rows, d.rank, d.target_score = ptr(scores), ptr(rows), ptr(rank), ptr(None if "s" in present else tscore)
    d.workspace, d.ws_bytes = ptr(ws), need
    d.Q, d.N, d.k, d.q_dtype, d.normalize_q, d.slab_rows = Q, N, k, _lib.F32, 0, SLAB
    x, g, t, c, b, s = (S["lthm_retrieve_" + n]() for n in ("excl", "group", "tags", "cursor", "bias", "shard"))
    x.rows, x.X = ptr(dv["excl"]), X
    g.G = G
    t.tags, t.filter = ptr(dv["tags"]), ptr(dv["filt"])
    keep += [torch.from_numpy(ref["asc"]).to(dev), torch.from_numpy(ref["arow"]).to(torch.int32).to(dev)]
    c.after_score, c.after_row = ptr(keep[-2]), ptr(keep[-1])
    b.bias, b.weight = ptr(dv["bias"]), ptr(dv["w"])
    s.target_score_in = ptr(tsin)
    parts = dict(x=x, g=g, t=t, c=c, b=b, s=s)
    args = [ctypes.addressof(parts[p]) if p in present else None for p in has]
    rc = getattr(lib, name)(ctypes.addressof(d), *args, stream())
    assert rc == 0, (name, rc)
    out = [scores.cpu().numpy().view(np.uint32), rows.cpu().numpy(), rank.cpu().numpy()]
    return out + [(tsin if "s" in present else tscore).cpu().numpy().view(np.uint32)], tscore


@pytest.mark.parametrize("name,has", ENTRIES)
def test_entry_point_is_the_general_call(dev, name, has):
    """Every scan entry point, given all the parts it takes, returns the bits of
    lthm_retrieve_topk_deep given the same parts (and of the checker's rows, so that the leg does
    compare lists).  The shard call is given the general call's target scores and then counts the
    general call's ranks: every target of this leg is a catalogue row."""
    present = has.replace("s", "")
    want, tscore = raw_call(dev, "lthm_retrieve_topk_deep", "xgtcb", present, 10)
    got, _ = raw_call(dev, name, has, has, 10, tsin=tscore if "s" in has else None)
    for a, e in zip(got, want):
        assert np.array_equal(a, e), name
    ref = reference("g" in has, "x" in has, "t" in has, "c" in has, "b" in has)
    assert np.array_equal(got[1], ref["rows"][:, :10]), name
    if name != "lthm_retrieve_topk_deep" and name != "lthm_retrieve_topk_shard":  # k <= 128 only, as ever
        from recommendations_amd import _lib
        d = _lib.STRUCTS["lthm_retrieve_desc"]()
        d.k = 129
        assert getattr(_lib.load(), name)(ctypes.addressof(d), *[None] * len(has), None) != 0


# ------------------------------------------------------------------ the timer's record
TIMED = [("retr_topk_k", False, "", 10), ("retr_topk_excl_k", False, "x", 10), ("retr_topk_tags_k", False, "xt", 10),
         ("retr_topk_after_k", False, "tc", 10), ("retr_topk_bias_k", False, "xtcb", 10),
         ("retr_topk_group_k", True, "x", 10), ("retr_topk_group_tags_k", True, "t", 10),
         ("retr_topk_group_after_k", True, "xc", 10), ("retr_topk_group_bias_k", True, "b", 10),
         ("retr_deep_topk_k", True, "xtcb", 200), ("retr_deep_topk_k", False, "", 129),
         ("retr_shard_topk_k", False, "xs", 10), ("retr_shard_topk_k", True, "tcbs", 200)]


@pytest.mark.parametrize("key,grouped,opts,k", TIMED)
def test_timer_record(dev, key, grouped, opts, k):
    """One call records one entry under the key of the narrowest entry point that takes it, with the
    flops of the scores and the bytes of the operands that are present."""
    from recommendations_amd import _lib
    from recommendations_amd import kernels as K
    x, t, c, b, ts = (o in opts for o in "xtcbs")
    dv, ref = on_device(dev), reference(grouped, x, t, c, b)
    fn, q = (K.retrieve_topk_group, dv["q3"]) if grouped else (K.retrieve_topk, dv["q1"])
    old, _lib.TIMER = _lib.TIMER, _lib.KernelTimer()
    try:
        fn(q, dv["items"], k, **kwargs(dv, ref, x, t, c, b, ts))
        records = _lib.TIMER.records
    finally:
        _lib.TIMER = old
    torch.cuda.synchronize()
    assert [r[0] for r in records] == [key]
    _, _, _, work, unit, nbytes = records[0]
    g = G if grouped else 1
    assert unit == "flop" and work == 2.0 * Q * g * N * D
    assert nbytes == (N * D * 2 + Q * g * D * 4 + Q * k * 8 + 4 * Q * X * x + (4 * N + 12 * Q) * t + 8 * Q * c
                      + (4 * N + 4 * Q) * b + 4 * Q * ts)
