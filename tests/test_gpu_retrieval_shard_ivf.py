"""Sharded clustered catalogues on the GPU (csrc/retrieve.hip lthm_retrieve_ivf_topk_shards,
K.retrieve_ivf_topk_shards, ShardedClusteredItemCatalogue): with every list probed the flat catalogue's
ids and score bits; with fewer the flat scan of the probed rows, and the f64 reference's id set; the fused
entry against one single-catalogue scan per shard and the merge; cursors and edge shapes; target ranks and
scores; guard rows; more probe slots than one call takes; the torch op; the wrapper; world 2.
The case is tests/retrieval_shard_ivf_case.py; the queries are unit-norm bf16 and go in with
normalize_q=False, so every kernel reads the reference's operands."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import retrieval_shard_ivf_case as C

pytestmark = pytest.mark.gpu

_CACHE = {}
ALL = 64  # at least every shard's nlist (7, 16, 1)


def bits(t):
    return t.contiguous().view(torch.int32)


def _same(got_ids, got_scores, want_ids, want_scores, what):
    assert torch.equal(got_ids.cpu(), want_ids.cpu()), what
    assert torch.equal(bits(got_scores.cpu()), bits(want_scores.cpu())), what


def env(kind="plain", with_bias=True):
    from recommendations_amd.models.lthm.sequence.retrieval import ShardedClusteredItemCatalogue
    dev = torch.device("cuda:0")
    if "case" not in _CACHE:
        _CACHE["case"] = C.build_case()
    key = (kind, with_bias)
    if key not in _CACHE:
        flat, sh = C.make_catalogues(_CACHE["case"], dev, with_bias, kind)
        _CACHE[key] = (flat, sh, ShardedClusteredItemCatalogue(sh), _CACHE["case"]["q"].to(dev))
    return (_CACHE["case"],) + _CACHE[key]


def _filter(dev):
    from recommendations_amd.models.lthm.sequence.retrieval import make_tag_filter
    g = torch.Generator().manual_seed(3)
    return make_tag_filter(C.Q, torch.randint(0, 4, (C.Q,), generator=g), 0, torch.randint(0, 4, (C.Q,), generator=g) << 4,
                           device=dev)


def _excludes(case, flat, q, dev):
    """int64 [Q, 40]: every query's 30 best items, five ids nobody holds and five pads."""
    best = flat.topk(q, 30, normalize_q=False)[0]
    return torch.cat([best, torch.full((C.Q, 5), 7, dtype=torch.int64, device=dev),
                      torch.zeros((C.Q, 5), dtype=torch.int64, device=dev)], dim=1).contiguous()


@pytest.mark.parametrize("k", [1, 10, 128])
def test_every_list_probed_plain_and_excluded(k):
    case, flat, sh, cat, q = env("plain", with_bias=False)
    ids, sc, rank, ts = cat.topk(q, k, nprobe=ALL, normalize_q=False)
    assert rank is None and ts is None
    want = flat.topk(q, k, normalize_q=False)
    _same(ids, sc, want[0], want[1], f"plain k={k}")
    ex = _excludes(case, flat, q, q.device)
    ids, sc, _, _ = cat.topk(q, k, nprobe=ALL, normalize_q=False, exclude_ids=ex)
    want = flat.topk(q, k, normalize_q=False, exclude_ids=ex)
    _same(ids, sc, want[0], want[1], f"excluded k={k}")
    assert not bool((ids[:, :, None] == ex[:, None, :30]).any())


@pytest.mark.parametrize("k", [1, 10, 128])
def test_every_list_probed_filters_and_prior(k):
    case, flat, sh, cat, q = env("filters")
    f = _filter(q.device)
    w = torch.linspace(-1, 2, C.Q, device=q.device)
    for kw in (dict(), dict(tag_filter=f), dict(bias_weight=0.5), dict(tag_filter=f, bias_weight=w)):
        ids, sc, _, _ = cat.topk(q, k, nprobe=ALL, normalize_q=False, **kw)
        want = flat.topk(q, k, normalize_q=False, **kw)
        _same(ids, sc, want[0], want[1], f"filters k={k} {sorted(kw)}")


def test_every_list_probed_deep():
    case, flat, sh, cat, q = env("deep")
    f = _filter(q.device)
    for kw in (dict(), dict(tag_filter=f, bias_weight=0.5)):
        ids, sc, _, _ = cat.topk(q, 1024, nprobe=ALL, normalize_q=False, **kw)
        want = flat.topk(q, 1024, normalize_q=False, **kw)
        _same(ids, sc, want[0], want[1], f"deep {sorted(kw)}")


def _probes(sh, q, nprobe):
    return [s.probe(q, min(nprobe, s.nlist), normalize_q=False).cpu().numpy() for s in sh]


@pytest.mark.parametrize("k", [1, 10, 128])
def test_partial_probe(k):
    case, flat, sh, cat, q = env("filters")
    mask = C.probed_mask(case, _probes(sh, q, 2))
    ids, sc, _, _ = cat.topk(q, k, nprobe=2, normalize_q=False, bias_weight=0.5)
    ref, decided = C.reference_topk(C.dense_scores(case, 0.5), mask, k)
    print(f"k={k}: tie rule leaves out {(~decided).mean():.4f} of the queries")
    assert (~decided).mean() <= C.CAP
    ids_np = case["ids"].numpy()
    for i in range(C.Q):
        rows = torch.from_numpy(np.nonzero(mask[i])[0]).to(q.device)
        want = flat.take(rows).topk(q[i:i + 1], k, normalize_q=False, bias_weight=0.5)
        _same(ids[i:i + 1], sc[i:i + 1], want[0], want[1], f"query {i} k={k}")
        if decided[i]:
            want_set = set(ids_np[ref[i][ref[i] >= 0]].tolist())
            assert set(ids[i][ids[i] != 0].tolist()) == want_set, f"query {i} k={k}: id set"


def test_cursor_pages():
    case, flat, sh, cat, q = env("filters")
    f = _filter(q.device)
    whole = cat.topk(q, 120, nprobe=2, normalize_q=False, tag_filter=f)
    cs = ci = None
    for page in range(3):
        ids, sc, _, _ = cat.topk(q, 40, nprobe=2, normalize_q=False, tag_filter=f, after_scores=cs, after_ids=ci)
        _same(ids, sc, whole[0][:, 40 * page:40 * page + 40], whole[1][:, 40 * page:40 * page + 40], f"page {page}")
        cs, ci = sc[:, -1].contiguous(), ids[:, -1].contiguous()


@pytest.mark.parametrize("kind,k", [("plain", 10), ("filters", 128), ("deep", 300)])
def test_fused_entry_against_the_loop(kind, k):
    from recommendations_amd import kernels as K
    case, flat, sh, cat, q = env(kind)
    f = _filter(q.device) if kind != "plain" else None
    ex = _excludes(case, flat, q, q.device)
    use_bias = kind != "plain"
    tup = [(s.emb, s.row_ids, s.list_off, s.centroids, s.tags, s.bias) for s in sh]
    xr = torch.stack([s.rows_of(ex) for s in sh]).contiguous()
    got = K.retrieve_ivf_topk_shards(q, tup, 2, k, normalize_q=False, exclude_rows=xr, tag_filter=f, use_bias=use_bias,
                                     bias_weight=0.5 if use_bias else None)
    ls, li = [], []
    for s in sh:
        if kind == "plain":
            a, b = s.topk(q, k, nprobe=min(2, s.nlist), normalize_q=False, exclude_ids=ex)
        else:
            a, b = s.topk(q, k, nprobe=min(2, s.nlist), normalize_q=False, exclude_ids=ex, tag_filter=f, bias_weight=0.5)
        ls.append(a)
        li.append(b)
    want = K.retrieve_merge_shards(torch.stack(ls).contiguous(), torch.stack(li).contiguous())
    assert got[2] is None
    _same(got[1], got[0], want[1], want[0], f"{kind} k={k}")


def test_edge_shapes():
    from recommendations_amd.models.lthm.sequence.retrieval import ShardedClusteredItemCatalogue, make_tag_filter
    case, flat, sh, cat, q = env("filters")
    # Q = 1
    ids, sc, _, _ = cat.topk(q[:1], 10, nprobe=ALL, normalize_q=False)
    want = flat.topk(q[:1], 10, normalize_q=False)
    _same(ids, sc, want[0], want[1], "Q = 1")
    # the one-row shard alone, and k past its row: (-inf, 0) behind it
    one = ShardedClusteredItemCatalogue([sh[2]])
    ids, sc, _, _ = one.topk(q, 5, nprobe=3, normalize_q=False)
    assert bool((ids[:, 0] == sh[2].row_ids[0]).all()) and bool((ids[:, 1:] == 0).all())
    assert bool(torch.isinf(sc[:, 1:]).all()) and bool((sc[:, 1:] < 0).all()) and bool(torch.isfinite(sc[:, 0]).all())
    # a filter no row of the one-row shard passes: that shard adds nothing, the others are unchanged
    t = int(sh[2].tags[0]) & 0xFFFF
    f = make_tag_filter(C.Q, 0, 0, t if t else 0, device=q.device)
    ids, sc, _, _ = cat.topk(q, 128, nprobe=ALL, normalize_q=False, tag_filter=f)
    want = flat.topk(q, 128, normalize_q=False, tag_filter=f)
    _same(ids, sc, want[0], want[1], "empty shard under the filter")
    if t:
        assert not bool((ids == sh[2].row_ids[0]).any())
    # a filter nothing passes: every slot is (-inf, 0)
    f = make_tag_filter(C.Q, 1, 0, 1, device=q.device)
    ids, sc, _, _ = cat.topk(q, 16, nprobe=2, normalize_q=False, tag_filter=f)
    assert bool((ids == 0).all()) and bool((sc == float("-inf")).all())
    # k above the eligible probed rows: the tail is (-inf, 0), the head the flat list of those rows
    f = make_tag_filter(C.Q, 0x3F, 0, 0, device=q.device)  # about 1 row in 64 passes
    ids, sc, _, _ = cat.topk(q, 128, nprobe=ALL, normalize_q=False, tag_filter=f)
    want = flat.topk(q, 128, normalize_q=False, tag_filter=f)
    _same(ids, sc, want[0], want[1], "k past the eligible rows")
    assert bool((ids[:, -1] == 0).all()) and bool((sc[:, -1] == float("-inf")).all())


def test_recall():
    case, flat, sh, cat, q = env("filters")
    assert cat.recall(q, 10, ALL) == 1.0
    r2, r4 = cat.recall(q, 10, 2), cat.recall(q, 10, 4)
    assert 0.0 < r2 <= r4 <= 1.0


def test_more_probe_slots_than_one_call_takes():
    """Five shards of 16 lists at nprobe = 16 are 80 probe slots: the entry refuses them in one call, the
    class makes two calls (4 + 1 shards) and merges, and with every list probed that is the flat list."""
    from recommendations_amd import kernels as K
    from recommendations_amd.models.lthm.sequence.retrieval import ClusteredItemCatalogue, ShardedClusteredItemCatalogue
    case, flat, _, _, q = env("filters")
    g = torch.Generator().manual_seed(4)
    sh = []
    for part in flat.split(5):
        cen = torch.nn.functional.normalize(torch.randn(16, 128, generator=g), dim=1).to(torch.bfloat16).to(q.device)
        sh.append(ClusteredItemCatalogue.from_assignment(part, cen, torch.randint(0, 16, (len(part),), generator=g))
                  .with_filters())
    cat = ShardedClusteredItemCatalogue(sh)
    assert [len(c) for c in cat._chunks(16)] == [4, 1] and [len(c) for c in cat._chunks(12)] == [5]
    tup = [(s.emb, s.row_ids, s.list_off, s.centroids, s.tags, s.bias) for s in sh]
    with pytest.raises(RuntimeError, match="probe slots of all shards together"):
        K.retrieve_ivf_topk_shards(q, tup, 16, 10, normalize_q=False)
    tid = case["ids"][::80][:C.Q].to(q.device)
    ids, sc, rk, ts = cat.topk(q, 100, nprobe=16, normalize_q=False, target_ids=tid, bias_weight=0.5)
    want = flat.topk(q, 100, normalize_q=False, target_ids=tid, bias_weight=0.5)
    _same(ids, sc, want[0], want[1], "two calls and a merge")
    assert torch.equal(rk, want[2].long()) and torch.equal(bits(ts), bits(want[3]))


def _targets(case, dev):
    g = torch.Generator().manual_seed(9)
    tid = case["ids"][torch.randint(0, C.N, (C.Q,), generator=g)].clone()
    tid[0], tid[1] = 5, case["ids"][-1]  # an id nobody holds; the item of the one-row shard
    return tid.to(dev)


@pytest.mark.parametrize("kind", ["plain", "filters", "deep"])
def test_target_rank_and_score(kind):
    case, flat, sh, cat, q = env(kind, with_bias=kind != "plain")
    tid = _targets(case, q.device)
    ex = _excludes(case, flat, q, q.device)
    kws = [dict(), dict(exclude_ids=ex)]
    if kind != "plain":
        kws += [dict(tag_filter=_filter(q.device), bias_weight=0.5, exclude_ids=ex)]
    for kw in kws:
        # every list probed: the flat catalogue's rank and target score
        k = 300 if kind == "deep" else 10
        ids, sc, rk, ts = cat.topk(q, k, nprobe=ALL, normalize_q=False, target_ids=tid, **kw)
        want = flat.topk(q, k, normalize_q=False, target_ids=tid, **kw)
        _same(ids, sc, want[0], want[1], f"{kind} {sorted(kw)}")
        assert rk.dtype == torch.int64 and torch.equal(rk, want[2].long()), (kind, sorted(kw))
        assert torch.equal(bits(ts), bits(want[3])), (kind, sorted(kw))
        assert int(rk[0]) == -1 and float(ts[0]) == float("-inf")
    # fewer lists: the flat rank of the probed rows plus the target, per query
    mask = C.probed_mask(case, _probes(sh, q, 2))
    ids, sc, rk, ts = cat.topk(q, 10, nprobe=2, normalize_q=False, target_ids=tid)
    full = flat.topk(q, 10, normalize_q=False, target_ids=tid)
    assert torch.equal(bits(ts), bits(full[3]))
    pos = {int(v): i for i, v in enumerate(case["ids"].tolist())}
    for i in range(C.Q):
        m = mask[i].copy()
        if int(tid[i]) in pos:
            m[pos[int(tid[i])]] = True
        rows = torch.from_numpy(np.nonzero(m)[0]).to(q.device)
        want = flat.take(rows).topk(q[i:i + 1], 10, normalize_q=False, target_ids=tid[i:i + 1])
        assert int(rk[i]) == int(want[2][0]), f"query {i}"
    # target_ranks: the plain dots unless a weight is given, as ItemCatalogue.target_ranks
    plain = ItemCatalogue_plain(flat)
    assert torch.equal(cat.target_ranks(q, tid, nprobe=ALL), plain.target_ranks(q, tid).long())


def ItemCatalogue_plain(flat):
    from recommendations_amd.models.lthm.sequence.retrieval import ItemCatalogue
    return ItemCatalogue(flat.ids, flat.emb, flat.tags)


def test_guard_rows_stay_untouched():
    """The entry writes [Q, k] scores and ids into the middle of larger buffers: the rows before and after
    keep their fill, for the shallow and the deep scan, with targets."""
    from recommendations_amd import kernels as K
    case, flat, sh, cat, q = env("deep")
    tup = [(s.emb, s.row_ids, s.list_off, s.centroids, s.tags, s.bias) for s in sh]
    tid = _targets(case, q.device)
    trows = torch.stack([s.rows_of(tid) for s in sh]).contiguous()
    tsc = flat.topk(q, 1, normalize_q=False, target_ids=tid)[3]
    tsc = torch.where(tsc == float("-inf"), torch.full_like(tsc, float("nan")), tsc).contiguous()
    for k in (7, 300):
        gs = torch.full((C.Q + 8, k), 12345.0, dtype=torch.float32, device=q.device)
        gi = torch.full((C.Q + 8, k), -777, dtype=torch.int64, device=q.device)
        out = (gs[4:4 + C.Q], gi[4:4 + C.Q])
        sc, ids, rk = K.retrieve_ivf_topk_shards(q, tup, 2, k, normalize_q=False, use_bias=True, target_rows=trows,
                                                 target_scores=tsc, out=out)
        torch.cuda.synchronize()
        assert bool((gs[:4] == 12345.0).all()) and bool((gs[4 + C.Q:] == 12345.0).all()), k
        assert bool((gi[:4] == -777).all()) and bool((gi[4 + C.Q:] == -777).all()), k
        ref = K.retrieve_ivf_topk_shards(q, tup, 2, k, normalize_q=False, use_bias=True)
        _same(ids, sc, ref[1], ref[0], f"guarded k={k}")
        assert rk.shape == (C.Q,) and bool((rk >= 0).all())


def test_torch_op_gives_the_kernel_wrapper_bits():
    from recommendations_amd import _lib
    from recommendations_amd import kernels as K
    _lib.load_torch_ops()
    case, flat, sh, cat, q = env("deep")
    f = _filter(q.device)
    tid = _targets(case, q.device)
    trows = torch.stack([s.rows_of(tid) for s in sh]).contiguous()
    tsc = flat.topk(q, 1, normalize_q=False, target_ids=tid)[3]
    tsc = torch.where(tsc == float("-inf"), torch.full_like(tsc, float("nan")), tsc).contiguous()
    tup = [(s.emb, s.row_ids, s.list_off, s.centroids, s.tags, s.bias) for s in sh]
    w = torch.full((C.Q,), 0.5, device=q.device)
    for k in (10, 300):
        want = K.retrieve_ivf_topk_shards(q, tup, 2, k, normalize_q=False, tag_filter=f, use_bias=True, bias_weight=w,
                                          target_rows=trows, target_scores=tsc)
        got = torch.ops.lthm.retrieve_ivf_topk_shards(q, [s.emb for s in sh], [s.row_ids for s in sh],
                                                      [s.list_off for s in sh], [s.centroids for s in sh],
                                                      [s.tags for s in sh], [s.bias for s in sh], 2, k, False, None, f,
                                                      True, w, None, None, trows, tsc)
        _same(got[1], got[0], want[1], want[0], f"op k={k}")
        assert torch.equal(got[2], want[2])
    got = torch.ops.lthm.retrieve_ivf_topk_shards(q, [s.emb for s in sh], [s.row_ids for s in sh], [s.list_off for s in sh],
                                                  [s.centroids for s in sh], [], [], 2, 10)
    want = K.retrieve_ivf_topk_shards(q, tup, 2, 10)
    _same(got[1], got[0], want[1], want[0], "op, plain")
    assert got[2].numel() == 0


def test_wrapper_gives_the_class_results():
    from lthm_step_case import build_wrapper, load_case
    from recommendations_amd.models.lthm.sequence.retrieval import ShardedClusteredItemCatalogue, build_catalogue
    dev = torch.device("cuda:0")
    fx, params, _, batch = load_case("lthm_step_a")
    m = build_wrapper(fx, params, dev).eval()
    b = {k: v.to(dev) for k, v in batch.items()}
    ids = batch["product_ids"].reshape(-1)
    extra = torch.randint(1, 2 ** 62, (300,), generator=torch.Generator().manual_seed(5))
    all_ids = torch.cat([extra, ids[ids != 0]])
    cat = build_catalogue(m, all_ids, chunk=128, tags=(all_ids % 5).to(torch.int32),
                          bias=((all_ids % 17).float() - 8.0) / 16.0)
    sh = ShardedClusteredItemCatalogue([p.cluster(4, iters=2).with_filters() for p in cat.split(3)])
    with torch.no_grad():
        out = m(b)
    q = out["next_token_emb"][:, -1, 0].contiguous()
    for kw, own in ((dict(), dict()), (dict(bias_weight=0.5, tag_any=3), None)):
        got = m.retrieve(b, sh, 20, nprobe=2, **kw)
        if own is None:
            from recommendations_amd.models.lthm.sequence.retrieval import make_tag_filter
            own = dict(bias_weight=0.5, tag_filter=make_tag_filter(q.shape[0], 0, 3, 0, device=dev))
        want = sh.topk(q if q.dtype in (torch.float32, torch.bfloat16) else q.float(), 20, nprobe=2, **own)
        _same(got["item_ids"], got["scores"], want[0], want[1], f"retrieve {sorted(kw)}")
    page = m.retrieve(b, sh, 10, nprobe=2, after=m.retrieve(b, sh, 10, nprobe=2))
    assert torch.equal(page["item_ids"], m.retrieve(b, sh, 20, nprobe=2)["item_ids"][:, 10:])
    # every list probed: the flat catalogue's metrics, key for key; fewer lists: the class's own ranks
    for kw in (dict(), dict(exclude_seen=True), dict(same_tags_mask=7), dict(bias_weight=0.5)):
        ref = m.catalogue_metrics(out, cat, **kw)
        got = m.catalogue_metrics(out, sh, nprobe=4, **kw)
        assert [v for k, v in ref.items() if k.startswith("catalogue_queries")][0] > 10
        assert list(got) == list(ref) and all(got[k] == ref[k] for k in ref), (kw, got, ref)
    part = m.catalogue_metrics(out, sh, nprobe=1)
    assert part["average_hit_position_catalogue"] <= m.catalogue_metrics(out, cat)["average_hit_position_catalogue"]


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_world2_matches_single_process(tmp_path):
    """tests/retrieval_shard_ivf_worker.py in one process (three shards, no group) and at world 2 (both
    ranks on this GPU over gloo; rank 0 holds shard {0}, rank 1 shards {1, 2}): both ranks get the
    single-process ids, score bits, ranks and target scores."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    worker = os.path.join(root, "tests", "retrieval_shard_ivf_worker.py")
    prefix = str(tmp_path / "shardivf")
    env_ = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    subprocess.run([sys.executable, worker, prefix], env=env_, check=True, timeout=240)
    subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                    "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), worker, prefix],
                   env=env_, check=True, timeout=240)
    w1 = torch.load(prefix + "_w1_r0.pt", weights_only=True)
    assert {"plain.ids", "all.rank", "partial.tscore", "holds", "filter"} <= set(w1)
    for r in range(2):
        w2 = torch.load(prefix + f"_w2_r{r}.pt", weights_only=True)
        assert set(w2) == set(w1)
        for key, a in w1.items():
            b = w2[key]
            assert a.dtype == b.dtype and a.shape == b.shape, (r, key)
            same = torch.equal(bits(a), bits(b)) if a.dtype == torch.float32 else torch.equal(a, b)
            assert same, (r, key)
