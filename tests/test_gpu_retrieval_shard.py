"""Sharded item catalogues (lthm_retrieve_target_score, lthm_retrieve_topk_shard,
lthm_retrieve_merge_shards; ShardedItemCatalogue): retrieval over id-partitioned shards, merged.

Definition under test: every output of the sharded call equals, bit for bit, the output of the
unsharded call on the union of the shards (ItemCatalogue.topk / K.retrieve_topk on the same device,
which the other retrieval tests pin to their fp64 checkers); rank alone changes its dtype to int64.
That holds because a (query, row) score does not depend on the tile, slab or shard the row sits in,
eligibility is per item, and ties break by id.  The merge kernel alone is held to the numpy model of
retrieval_shard_case.py (itself checked on the host).

N = 3,000 is 46 tiles + 56 rows and Q = 70 two query tiles, the second partial.  The integer case
(operands in {-1, 0, 1}, 48 distinct rows repeated, normalize_q=False, slab_rows=64) has every score
in a tie run that crosses every shard boundary; the unit-vector case goes through normalize_q."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist

from lthm_step_case import build_wrapper, load_case
from retrieval_shard_case import N, Q, case, merge_case, merge_model

pytestmark = pytest.mark.gpu

_CACHE = {}


def bits(t):
    return None if t is None else (t.view(torch.int32) if t.dtype == torch.float32 else t).cpu()


def same(a, b, what=""):
    """Two result tuples, bit for bit; an integer rank may differ in width only."""
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert (x is None) == (y is None), (what, i)
        if x is None:
            continue
        if not x.is_floating_point():
            x, y = x.long(), y.long()
        assert x.shape == y.shape and torch.equal(bits(x), bits(y)), (what, i)


# ------------------------------------------------------------------ 1. the merge kernel alone
@pytest.mark.parametrize("k", [1, 63, 64, 65, 128, 129, 1024])
@pytest.mark.parametrize("S", [1, 2, 3, 8, 64])
def test_merge_kernel_against_the_model(dev, S, k):
    from recommendations_amd import kernels as K
    scores, ids, ranks = merge_case(S, k)
    ref_s, ref_i, ref_r = merge_model(scores, ids, ranks)
    ts, ti, tr = torch.from_numpy(scores).to(dev), torch.from_numpy(ids).to(dev), torch.from_numpy(ranks).to(dev)
    got_s, got_i, got_r = K.retrieve_merge_shards(ts, ti, tr)
    assert got_r.dtype == torch.int64 and got_i.dtype == torch.int64
    assert torch.equal(got_i.cpu(), torch.from_numpy(ref_i))
    assert torch.equal(bits(got_s), torch.from_numpy(ref_s).view(torch.int32))
    assert torch.equal(got_r.cpu(), torch.from_numpy(ref_r))
    assert bool((ref_r == -1).any()) and bool((ref_r >= 0).any())
    # ranks without a -1, and no ranks at all
    r2 = np.abs(ranks)
    got = K.retrieve_merge_shards(ts, ti, torch.from_numpy(r2).to(dev))
    assert torch.equal(got[2].cpu(), torch.from_numpy(r2.astype(np.int64).sum(0)))
    got = K.retrieve_merge_shards(ts, ti)
    assert got[2] is None and torch.equal(got[1], got_i) and torch.equal(bits(got[0]), bits(got_s))
    from recommendations_amd import _lib
    _lib.load_torch_ops()
    s2, i2, r2t = torch.ops.lthm.retrieve_merge_shards(ts, ti, tr)
    assert torch.equal(i2, got_i) and torch.equal(bits(s2), bits(got_s)) and torch.equal(r2t, got_r)


def test_merge_kernel_refuses(dev):
    from recommendations_amd import kernels as K
    z = torch.zeros((2, 3, 4), device=dev)
    for s, i, r in ((z[:0], z[:0].long(), None), (torch.zeros((65, 1, 2), device=dev), torch.zeros((65, 1, 2), device=dev).long(), None),
                    (torch.zeros((2, 1, 1025), device=dev), torch.zeros((2, 1, 1025), device=dev).long(), None),
                    (z, z.int(), None), (z, z.long(), torch.zeros((2, 3), device=dev).long())):
        with pytest.raises((ValueError, RuntimeError)):
            K.retrieve_merge_shards(s, i, r)


# ------------------------------------------------------------------ 2. the target score
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("normalize_q", [False, True])
@pytest.mark.parametrize("qdt", [torch.float32, torch.bfloat16])
def test_target_score_equals_the_scans(dev, qdt, normalize_q, G, with_bias):
    from recommendations_amd import kernels as K
    c = case("unit")
    items = c["emb"].to(dev)
    q = (c["q"] if G == 1 else c["q3"]).to(qdt).to(dev)
    trow = ((torch.arange(Q) * 7919 + 3) % N).to(torch.int32)
    trow[0], trow[1], trow[2], trow[3] = -1, N, 0, N - 1
    trow = trow.to(dev)
    kw = dict(bias=c["bias"].to(dev), bias_weight=c["bw"].to(dev)) if with_bias else {}
    fn = K.retrieve_topk if G == 1 else K.retrieve_topk_group
    ref = fn(q, items, 5, normalize_q=normalize_q, target_rows=trow, **kw)[3]
    got = K.retrieve_target_score(q, items, trow, normalize_q=normalize_q, **kw)
    ok = (trow >= 0) & (trow < N)
    assert torch.equal(bits(got)[ok.cpu()], bits(ref)[ok.cpu()])
    assert bool(torch.isnan(got[~ok]).all()) and int((~ok).sum()) == 2 and not bool(torch.isnan(got[ok]).any())
    if with_bias:  # weight None is 1
        ref1 = fn(q, items, 5, normalize_q=normalize_q, target_rows=trow, bias=kw["bias"])[3]
        got1 = K.retrieve_target_score(q, items, trow, normalize_q=normalize_q, bias=kw["bias"])
        assert torch.equal(bits(got1)[ok.cpu()], bits(ref1)[ok.cpu()])


# ------------------------------------------------------------------ 3. the shard mode of the scan
@pytest.mark.parametrize("k", [100, 300])
@pytest.mark.parametrize("kind", ["int", "unit"])
def test_scan_counts_against_given_scores(dev, kind, k):
    """The target's row replaced by -1 and its score handed in: scores and rows do not change, and
    rank grows by one exactly where the target's own MFMA score is strictly above the score handed
    in (the target is then one more row above it; with the row given it is left out by row)."""
    from recommendations_amd import kernels as K
    c = case(kind)
    items, q = c["emb"].to(dev), c["q"].to(dev)
    norm = kind == "unit"
    trow = ((torch.arange(Q) * 7919 + 3) % N).to(torch.int32)
    trow[::5] = -1
    trow = trow.to(dev)
    valid = trow >= 0
    full = K.retrieve_topk(q, items, k, normalize_q=norm, target_rows=trow, slab_rows=64, deep=True)
    ts_in = torch.where(valid, full[3], torch.full_like(full[3], float("nan")))
    # the same rows given: the same four outputs, with the NaN queries at rank -1
    got = K.retrieve_topk(q, items, k, normalize_q=norm, target_rows=trow, slab_rows=64, deep=True, target_scores=ts_in)
    same(got[:3], full[:3], "rows given")
    assert got[3] is ts_in
    # the target's own MFMA score, from a scan of the catalogue of the 70 target rows (a score does
    # not depend on where its row sits): entry q of query q
    t_items = items[trow.clamp(min=0).long()]
    s_all, r_all, _, _ = K.retrieve_topk(q, t_items, Q, normalize_q=norm)
    own = s_all[r_all == torch.arange(Q, device=dev, dtype=torch.int32)[:, None]]  # one entry per query, in order
    assert own.shape == (Q,)
    plus = (valid & (own > full[3])).int()
    print(f"{kind} k={k}: {int(plus.sum())} targets score strictly below their own MFMA score")
    for tr in (torch.full_like(trow, -1), None):
        got = K.retrieve_topk(q, items, k, normalize_q=norm, target_rows=tr, slab_rows=64, deep=True, target_scores=ts_in)
        same(got[:2], full[:2], "rows hidden")
        assert got[2].dtype == torch.int32
        assert torch.equal(got[2], torch.where(valid, full[2] + plus, torch.full_like(full[2], -1)))
    if kind == "int":
        assert int(plus.sum()) == 0  # exact arithmetic: the dot and the MFMA agree


# ------------------------------------------------------------------ 4. sharded against unsharded
def catalogues(dev, kind):
    """(plain, rich): the union without and with tags and bias, on the device."""
    from recommendations_amd.models.lthm.sequence.retrieval import ItemCatalogue
    key = ("cat", kind)
    if key not in _CACHE:
        c = case(kind)
        _CACHE[key] = (ItemCatalogue(c["ids"].to(dev), c["emb"].to(dev)),
                       ItemCatalogue(c["ids"].to(dev), c["emb"].to(dev), c["tags"].to(dev), c["bias"].to(dev)))
    return _CACHE[key]


PLANS = ["split1", "split3", "split7", "interleaved", "tiny"]


def shards_of(cat, plan):
    n = len(cat)
    rows = torch.arange(n, device=cat.ids.device)
    if plan.startswith("split"):
        return cat.split(int(plan[5:]))
    if plan == "interleaved":  # ties alternate between the shards
        return [cat.take(rows % 3 == r) for r in range(3)]
    # one 1-row shard in the middle, one shard with fewer rows than any k but 1, the rest
    return [cat.take(rows == 1500), cat.take((rows < 60) & (rows != 1500)), cat.take((rows >= 60) & (rows != 1500))]


def cursor(dev, kind, rich, kw):
    """A cursor per query inside the reference list: entry 30 + q of the k = 128 list."""
    full = catalogues(dev, kind)[rich]
    ids, scores, _, _ = full.topk(**kw, k=128)
    pos = (30 + torch.arange(Q, device=dev))[:, None]
    return scores.gather(1, pos)[:, 0].contiguous(), ids.gather(1, pos)[:, 0].contiguous()


def variants(dev, kind):
    """name -> (uses the rich catalogue, topk keywords)"""
    key = ("var", kind)
    if key not in _CACHE:
        c = {n: v.to(dev) for n, v in case(kind).items()}
        base = dict(normalize_q=kind == "unit", slab_rows=64 if kind == "int" else 0)
        v = {
            "plain": (False, dict(q=c["q"], **base)),
            "targets": (False, dict(q=c["q"], target_ids=c["target_ids"], **base)),
            "exclude": (False, dict(q=c["q"], exclude_ids=c["exclude_ids"], target_ids=c["target_ids"], **base)),
            "group": (False, dict(q=c["q3"], target_ids=c["target_ids"], **base)),
            "tags": (True, dict(q=c["q"], tag_filter=c["filt"], target_ids=c["target_ids"], **base)),
            "bias": (True, dict(q=c["q"], bias_weight=c["bw"], target_ids=c["target_ids"], **base)),
        }
        cs, ci = cursor(dev, kind, False, dict(q=c["q"], **base))
        v["after"] = (False, dict(q=c["q"], after_scores=cs, after_ids=ci, target_ids=c["target_ids"], **base))
        every = dict(q=c["q3"], target_ids=c["target_ids"], exclude_ids=c["exclude_ids"], tag_filter=c["filt"],
                     bias_weight=c["bw"], **base)
        cs, ci = cursor(dev, kind, True, every)
        v["all"] = (True, dict(after_scores=cs, after_ids=ci, **every))
        _CACHE[key] = v
    return _CACHE[key]


def reference(dev, kind, name, k):
    key = ("ref", kind, name, k)
    if key not in _CACHE:
        rich, kw = variants(dev, kind)[name]
        _CACHE[key] = catalogues(dev, kind)[rich].topk(k=k, **kw)
    return _CACHE[key]


@pytest.mark.parametrize("k", [1, 100, 128, 129, 1024])
@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("kind", ["int", "unit"])
def test_sharded_equals_unsharded(dev, kind, plan, k):
    from recommendations_amd.models.lthm.sequence.retrieval import ShardedItemCatalogue
    sharded = [ShardedItemCatalogue(shards_of(cat, plan)) for cat in catalogues(dev, kind)]
    assert len(sharded[0]) == N
    for name, (rich, kw) in variants(dev, kind).items():
        ref = reference(dev, kind, name, k)
        got = sharded[rich].topk(k=k, **kw)
        assert got[2] is None or got[2].dtype == torch.int64
        same(got, ref, (kind, plan, k, name))
        if "target_ids" in kw:  # ids that no shard holds: no target
            assert bool((got[2][::5] == -1).all()) and bool((got[3][::5] == float("-inf")).all())


def test_paging_through_shards(dev):
    """Three pages of 100 through a sharded catalogue are the first 300 of one k = 300 call, sharded
    and unsharded."""
    from recommendations_amd.models.lthm.sequence.retrieval import ShardedItemCatalogue
    for kind in ("int", "unit"):
        rich, kw = variants(dev, kind)["all"]
        kw = {n: v for n, v in kw.items() if not n.startswith("after")}
        full = catalogues(dev, kind)[rich]
        sh = ShardedItemCatalogue(shards_of(full, "interleaved"))
        whole = sh.topk(k=300, **kw)
        same(whole, full.topk(k=300, **kw), kind)
        pages, after = [], {}
        for _ in range(3):
            p = sh.topk(k=100, **kw, **after)
            pages.append(p)
            after = dict(after_scores=p[1][:, -1].contiguous(), after_ids=p[0][:, -1].contiguous())
        assert torch.equal(torch.cat([p[0] for p in pages], 1), whole[0])
        assert torch.equal(bits(torch.cat([p[1] for p in pages], 1)), bits(whole[1]))


# ------------------------------------------------------------------ 5. the wrapper
def _model_case(dev):
    if "model" not in _CACHE:
        from recommendations_amd.models.lthm.sequence.retrieval import build_catalogue
        fx, params, _, batch = load_case("lthm_step_a")
        m = build_wrapper(fx, params, dev).eval()
        b = {k: v.to(dev) for k, v in batch.items()}
        ids = batch["product_ids"].reshape(-1)
        extra = torch.randint(1, 2 ** 62, (300,), generator=torch.Generator().manual_seed(5))
        all_ids = torch.cat([extra, ids[ids != 0]])
        cat = build_catalogue(m, all_ids, chunk=128, tags=(all_ids % 5).to(torch.int32),
                              bias=((all_ids % 17).float() - 8.0) / 16.0)
        with torch.no_grad():
            out = m(b)
        _CACHE["model"] = (m, b, out, cat)
    return _CACHE["model"]


def test_wrapper_through_shards(dev):
    from recommendations_amd.models.lthm.sequence.retrieval import ShardedItemCatalogue
    m, b, out, cat = _model_case(dev)
    sh = ShardedItemCatalogue(cat.split(3))
    B = b["product_ids"].shape[0]
    wt = torch.linspace(-1.0, 2.0, B)
    for kw in (dict(), dict(exclude_history=True), dict(bias_weight=0.5), dict(tag_any=3),
               dict(bias_weight=wt, exclude_history=True, heads=[0, 2], tag_none=4)):
        for k in (20, 200):
            ref = m.retrieve(b, cat, k, **kw)
            got = m.retrieve(b, sh, k, **kw)
            assert torch.equal(got["item_ids"], ref["item_ids"]), kw
            assert torch.equal(bits(got["scores"]), bits(ref["scores"])), kw
        page = m.retrieve(b, sh, 20, after=m.retrieve(b, sh, 20, **kw), **kw)
        ref = m.retrieve(b, cat, 40, **kw)
        assert torch.equal(page["item_ids"], ref["item_ids"][:, 20:])
    for kw in (dict(), dict(exclude_seen=True), dict(same_tags_mask=7), dict(bias_weight=0.5),
               dict(exclude_seen=True, same_tags_mask=7, bias_weight=0.5, head=1, ks=[1, 5, 20])):
        ref = m.catalogue_metrics(out, cat, **kw)
        got = m.catalogue_metrics(out, sh, **kw)
        assert [v for k, v in ref.items() if k.startswith("catalogue_queries")][0] > 10
        assert list(got) == list(ref) and all(got[k] == ref[k] for k in ref), (kw, got, ref)


# ------------------------------------------------------------------ 6. process groups
@pytest.fixture
def rccl1(dev):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    store = dist.TCPStore("127.0.0.1", port, 1, True)
    dist.init_process_group("nccl", store=store, rank=0, world_size=1, device_id=dev)
    try:
        yield
    finally:
        dist.destroy_process_group()


def test_world1_group_equals_groupless(dev, rccl1):
    from recommendations_amd.models.lthm.sequence.retrieval import ShardedItemCatalogue
    full = catalogues(dev, "int")[1]
    rich, kw = variants(dev, "int")["all"]
    a = ShardedItemCatalogue([full], group=dist.group.WORLD)
    b = ShardedItemCatalogue([full])
    a.validate()
    assert len(a) == len(b) == N
    for k in (100, 300):
        same(a.topk(k=k, **kw), b.topk(k=k, **kw), k)
        same(a.topk(k=k, **kw), reference(dev, "int", "all", k), k)
    ids = case("int")["target_ids"].to(dev)
    assert torch.equal(a.filter_like(ids, 7), full.filter_like(ids, 7))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_world2_matches_world1(dev, tmp_path):
    """tests/retrieval_shard_worker.py at world 1 (one unsharded catalogue) and at world 2 (both ranks
    on this GPU over gloo, each holding half of the catalogue): topk with every option at k = 100
    and k = 300, and build_catalogue(shard=(rank, 2)) on the row-sharded item table against the
    world-1 catalogue.  emb is a gather and a fixed-order sum, so it is expected bit for bit; where
    it is not, every element is within one bf16 ulp (two bf16 roundings of f32 values that differ
    in summation order only)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    worker = os.path.join(root, "tests", "retrieval_shard_worker.py")
    prefix = str(tmp_path / "shard")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    subprocess.run([sys.executable, worker, prefix], env=env, check=True, timeout=240)
    subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                    "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), worker, prefix],
                   env=env, check=True, timeout=240)
    w1 = torch.load(prefix + "_w1_r0.pt", weights_only=True)
    w2 = [torch.load(prefix + f"_w2_r{r}.pt", weights_only=True) for r in range(2)]
    for key in w1:
        if key.startswith("topk."):
            for r in range(2):
                assert w2[r][key].dtype == w1[key].dtype or key.endswith(".rank")
                assert torch.equal(bits(w2[r][key].long() if key.endswith(".rank") else w2[r][key]),
                                   bits(w1[key].long() if key.endswith(".rank") else w1[key])), (key, r)
    n = w1["cat.ids"].numel()
    lo = 0
    for r in range(2):
        hi = (r + 1) * n // 2
        assert torch.equal(w2[r]["cat.ids"], w1["cat.ids"][lo:hi]), r  # the slice bounds, exactly
        assert torch.equal(w2[r]["cat.tags"], w1["cat.tags"][lo:hi]) and torch.equal(w2[r]["cat.bias"], w1["cat.bias"][lo:hi])
        a, b = w2[r]["cat.emb"], w1["cat.emb"][lo:hi]
        differ = int((a.view(torch.int16) != b.view(torch.int16)).sum())
        print(f"rank {r}: {differ} of {a.numel()} catalogue elements differ from world 1")
        if differ:
            ulp = torch.maximum(a.float().abs(), b.float().abs()) * 2.0 ** -7  # one bf16 ulp is at most 2^-7 |x|
            assert bool(((a.float() - b.float()).abs() <= ulp).all())
        lo = hi
    assert lo == n
