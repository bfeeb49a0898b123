"""Full-catalogue retrieval benchmark: K.retrieve_topk against the torch baseline
``(q_bf16 @ items.T).float().topk(k)`` on the same device and inputs.

    python tools/bench_retrieval.py [--shapes serving,evaluation] [--reps 20] [--n-items 2000000] [--exclude X]
                                    [--group G] [--tags P] [--after] [--deep K] [--bias]
    python tools/bench_retrieval.py --shards S [--shapes ...] [--reps 20] [--n-items 2000000] [--k 100]
    python tools/bench_retrieval.py --ivf L [--shapes ...] [--reps 20] [--n-items 2000000] [--k 100]
    python tools/bench_retrieval.py --ivf-heads L [--group 3] [--shapes ...] [--reps 20] [--n-items 2000000] [--k 100]

Each shape runs in a child process of its own (checked exit status, time limit); a failed
shape stops the run.  One JSON line per shape:
  fused_ms / base_ms      median device time of one call (HIP events; the fused call is its
                          three launches: prep, scores + selection, merge), with min / max
  *_floor_frac            the least time the hardware could take over the measured time, the
                          floor being max(catalogue + query + output bytes / 8.0 TB/s,
                          2 Q N 128 flop / 2.5 Pflop/s); ``bound`` names the larger term
  speedup, speedup_lo     base / fused on the medians, and on the worst pairing (base min /
                          fused max): faster only if speedup_lo > 1
  check_rows_equal        the fused rows of the first queries equal an f32 torch top-k's
  excl_* (--exclude X)    the fused call with X random valid rows excluded per query
                          (exclude_rows), timed next to the plain one: median / min / max,
                          excl_over_fused = excl / fused on the medians (_hi: excl max / fused
                          min), and its rows against a torch top-k with those rows at -inf
  group_* (--group G)     U = Q // G users of G queries each (Q becomes U G): the grouped call
                          (K.retrieve_topk_group) timed next to the plain call on the same U G
                          queries (fused_*) and next to what a caller without it does, G plain calls
                          of U queries and a merge of the G lists with torch sorts on the device
                          (heads_*): group_over_fused and group_over_heads on the medians (_hi /
                          _lo: the worst pairing), group_check_rows_equal against that merge
  tags_* (--tags P)       random tags such that a fraction P of the rows is eligible for every query
                          (bit 0 set with probability P, every query's filter (1, 0, 0)): the filtered
                          call timed next to the plain one, tags_over_fused on the medians (_hi: the
                          worst pairing), its rows against a torch top-k with the ineligible rows at
                          -inf.  With --exclude also the excluding + filtered call (xtags_*, over the
                          plain call), with --group the grouped + filtered call (gtags_*, over the
                          plain and over the grouped call)
  after_* (--after)       page 2 of k rows (the call with page 1's last (score, row) as its cursor) timed
                          next to page 1, the plain call: after_over_fused on the medians (_hi: the worst
                          pairing), its rows against entries k .. 2k - 1 of a torch top-2k
  deep_* (--deep K)       the deep list of K rows, deep=True (one catalogue scan: deep_ms = deep_scan_ms),
                          against deep="paged" (deep_paged_*: ceil(K / 128) passes, one catalogue scan each)
                          and the baseline's top-K (deep_base_*), all in the same loop: deep_scan_over_paged on
                          the medians (_hi: the worst pairing, scan max / paged min; faster only if < 1),
                          deep_over_base (_hi), deep_over_fused against the plain call;
                          deep_check_rows_equal: the fraction of the single scan's (score bits, rows) of all
                          queries equal to the paged arm's (1.0: the same lists); deep_check_rows_equal_torch:
                          its rows of the first queries against an f32 torch top-K
  bias_* (--bias)         the call with a random f32 bias per row (uniform in [-0.05, 0.05], the scale of
                          the scores' spread) and weight 1, timed next to the plain one: bias_over_fused on
                          the medians (_hi: the worst pairing), its rows against a torch top-k of
                          scores + bias
--shards S is a mode of its own (no torch baseline): the catalogue as S contiguous shards on this device
in a ShardedItemCatalogue, whose topk (with targets: S target-score calls, S scans, one merge) is timed
next to the one unsharded call with targets, in the same loop, beside the target-score call alone and
the merge kernel alone on the S lists of k rows and on S synthetic full lists of 1,024:
  unsharded_ms / sharded_ms        medians (min / max), sharded_minus_unsharded_ms their difference
  tscore_ms, merge_ms, merge_1024_ms   the S target-score calls of the shards; the merge launch alone
  merge_floor_ms                   S Q k 12 B read + Q k 12 B written at 8.0 TB/s
  scans_ms                         the S shard scans alone (the sharded call without steps 1, 2, 4, 5)
  check_equal                      the sharded call's four outputs equal the unsharded call's, bit for bit
--ivf L is a mode of its own too: N items drawn around 4,096 random unit centres (normalize(centre +
0.7 noise / sqrt(128)); uniform random vectors have no lists worth probing), the queries drawn the same
way, the catalogue clustered into L lists (ItemCatalogue.cluster, 5 iterations on a sample of 262,144
rows; build_s is reported, not judged).  One JSON line per nprobe in {1, 8, 32, 64}:
  flat_ms / ivf_ms            the flat call and ClusteredItemCatalogue.topk (probe scan + the clustered call),
                              medians (min / max) of the same alternating loop, and ivf_over_flat (_hi: ivf max /
                              flat min; faster only if < 1)
  probe_ms, scan_call_ms, merge_ms   the probe scan alone (K.retrieve_topk over the centroids), the one C call
                              behind it alone (prep, plan, list scan, merge) and the merge launch alone on P lists
  plan_us, list_scan_us, merge_us    device time of the call's own kernels from one profiled call (the three plan
                              kernels summed; null where the profiler gives nothing)
  recall_at_k, rows_per_query the mean fraction of the flat top-k returned, the mean rows a query scans (of N)
--ivf-filt L is a mode of its own too: the catalogue of --ivf with one random tag bit (half the rows carry it)
and a random finite bias per row.  One JSON line per nprobe in {1, 8, 32}, four arms in one alternating loop,
medians (min / max):
  plain_ms                    ClusteredItemCatalogue.topk, the unfiltered scan (tags and bias ignored)
  neutral_ms                  the with_filters() view with the filter (0, 0, 0) and weight 0: the cost of the machinery
  filt_ms                     the view with tag_all = the bit (50 % selective) and weight 1
  flat_ms                     to_flat().topk with that filter and weight: what the flat path costs
  neutral_over_plain, filt_over_plain, filt_over_flat (and _hi, the worst pairing: max / min)
  neutral_equals_plain, filt_equals_flat_on_probed   the arms' outputs checked where the contract makes them equal
With --baseline-lib PATH (another build of liblthm_hip.so, say the parent commit's) a fifth and sixth arm time the
one C call lthm_retrieve_ivf_topk of that library and of this one on the same probes (base_scan_call_ms,
scan_call_ms, scan_call_over_base): the unfiltered path's timing against its parent in the same loop.
--ivf-deep L is a mode of its own too: the catalogue of --ivf with random group keys, its with_deep() view.  One JSON
line per (shape, nprobe in {8, 32}, k in {256, 1024}), all arms alternating in one loop, medians (min / max):
  ivf_deep_ms / flat_deep_ms  the view's topk (probe scan + the deep clustered call) and the flat deep call with the same
                              k; deep_over_flat on the medians (_hi: the worst pairing, ivf max / flat min; faster only if
                              < 1); deep_equals_flat_on_probed (the flat list's entries that lie in a probed list are, bit
                              for bit and in order, the head of the clustered list; the first 64 queries) and recall_at_k
With --baseline-lib PATH two more arms time lthm_retrieve_ivf_topk at k = 100 through that library and through this one
(scan_call_within_base: each median inside the other's min-max range).  The serving shape adds one line per nprobe for
the chain deep pool of 1,024 -> diversify k = 100 (lam 0.7, group_cap 2), the view against the flat catalogue.
--ivf-heads L is a mode of its own too: the catalogue of --ivf, U users of G = --group (default 3) queries each, every
query drawn around a centre of its own, nprobe = 8.  One JSON line per shape, three arms alternating in one loop,
medians (min / max):
  ivf_heads_ms                the with_heads() view's topk: the grouped probe scan + lthm_retrieve_ivf_topk_group
  flat_group_ms               K.retrieve_topk_group over the whole catalogue; heads_over_flat (_hi: the worst pairing,
                              heads max / flat min; faster only if < 1)
  separate_ms                 G ClusteredItemCatalogue.topk calls, one per head with its own 8 probes, and a torch merge
                              that removes an id's duplicates (merge_heads); heads_over_separate
  recall_at_k, separate_recall_at_k   the mean fraction of the flat grouped call's top-k each returns; rows_per_user and
                              separate_rows_per_user the rows either scans per user; no_item_twice
--diversify is a mode of its own too: Q = 256 queries, N unit rows drawn as --ivf draws them, the pool the deep
scan's own first M rows for M in {512, 1024}, k = 100 by default, lam = 0.7.  One JSON line per M:
  kernel_ms / torch_ms        K.retrieve_diversify and a torch greedy loop on the device over the gathered
                              [Q, M, 128] f32 rows (k steps of mask, argmax, gather, batched dot, maximum), medians
                              (min / max) of the same alternating loop, and kernel_over_torch (_hi: kernel max /
                              torch min; faster only if < 1)
  fma_per_s                   Q k M 128 multiply-adds over the kernel's median
  same_rows                   the fraction of list slots where the two agree (near-ties may fall either way)
--q8 POOL is a mode of its own too: the e4m3 catalogue of the rows --ivf draws.  One JSON line per shape:
  flat_deep_ms / q8_scan_ms   K.retrieve_topk(k = POOL, deep=True), the bf16 way to such a shortlist, and
                              K.retrieve_q8_topk(pool = POOL), with q8_scan_over_flat_deep (faster only if < 1)
  q8_two_stage_ms / flat_ms   the e4m3 scan plus K.retrieve_rescore to k, and the flat call at k, with
                              q8_two_stage_over_flat; torch_ms is the baseline at k
  bf16_bytes_per_scan, q8_bytes_per_scan   catalogue bytes one scan reads (256 B and 128 + 4 B per row)
  recall_at_k (_min)          the mean (least) fraction of the flat top-k the two-stage list returns
--ivf-q8 L is a mode of its own too: --ivf's catalogue with a tag bit on half the rows and a N(0, 0.05) bias, its
quantize()d twin, nprobe 8, tag_all = 1, bias_weight 1.  One JSON line per (shape, pool in {256, 1024}), medians (min / max):
  bf16_deep_ms / q8_scan_ms   the with_deep() view's topk at k = pool and QuantizedClusteredItemCatalogue.topk(pool,
                              rescore=False), both with their probe scan: q8_scan_over_bf16_deep (_hi: the worst
                              pairing, q8 max / bf16 min; faster only if < 1)
  q8_two_stage_ms / bf16_filt_ms   the e4m3 scan at pool plus the re-scoring to k = 100, and the with_filters() view at
                              k = 100: q8_two_stage_over_bf16_filt (_hi)
  bytes_per_row_*             arithmetic: codes + scale (132 B) or bf16 rows (256 B), plus row id, tag and bias words
  recall_at_100               the mean fraction of the bf16 clustered list the two-stage list returns
The paths alternate inside the timed loop.  Shapes: serving Q = 256, evaluation Q = 4096
(baseline chunked over Q so that its score matrix fits), N = 2,000,000, k = 100.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12     # B/s, spec
MFMA_PEAK = 2.5e15    # bf16 flop/s, dense, spec
SHAPES = {"serving": 256, "evaluation": 4096}
BASE_CHUNK = 256      # baseline queries per matmul: a [256, N] f32 score matrix is 2 GB at N = 2M


def merge_heads(lists, k):
    """G per-head (scores [U, k], rows [U, k]) -> the k best distinct rows per user by (best score
    descending, row ascending), with stable sorts: by score, by row, the duplicates out, by score."""
    import torch
    sc = torch.cat([x[0] for x in lists], dim=1)
    rw = torch.cat([x[1] for x in lists], dim=1)
    o = sc.argsort(dim=1, descending=True, stable=True)
    sc, rw = sc.gather(1, o), rw.gather(1, o)
    o = rw.argsort(dim=1, stable=True)
    sc, rw = sc.gather(1, o), rw.gather(1, o)  # equal rows adjacent, the best score first
    sc[:, 1:] = torch.where(rw[:, 1:] == rw[:, :-1], torch.full_like(sc[:, 1:], float("-inf")), sc[:, 1:])
    o = sc.argsort(dim=1, descending=True, stable=True)[:, :k]
    return sc.gather(1, o), rw.gather(1, o)


def child(name: str, N: int, k: int, reps: int, exclude: int = 0, group: int = 0, tags_p: float = -1.0,
          after: bool = False, deep: int = 0, bias: bool = False) -> None:
    import torch
    from recommendations_amd import kernels as K
    Q = SHAPES[name]
    if group:
        Q = Q // group * group
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    items = torch.empty((N, 128), dtype=torch.bfloat16, device=dev)
    for lo in range(0, N, 1 << 18):  # normalised random rows, built in pieces
        x = torch.randn((min(1 << 18, N - lo), 128), generator=g, device=dev)
        items[lo:lo + x.shape[0]] = torch.nn.functional.normalize(x, dim=-1).to(torch.bfloat16)
    q = torch.nn.functional.normalize(torch.randn((Q, 128), generator=g, device=dev), dim=-1)
    q_bf = q.to(torch.bfloat16)

    def fused():
        return K.retrieve_topk(q_bf, items, k, normalize_q=False)

    xr = None
    if exclude:  # X random valid rows per query
        xr = torch.randint(0, N, (Q, exclude), generator=g, device=dev, dtype=torch.int32)

    def fused_excl():
        return K.retrieve_topk(q_bf, items, k, normalize_q=False, exclude_rows=xr)

    q_grp, q_heads = None, []
    if group:
        q_grp = q_bf.view(Q // group, group, 128)
        q_heads = [q_grp[:, h].contiguous() for h in range(group)]

    def fused_group():
        return K.retrieve_topk_group(q_grp, items, k, normalize_q=False)

    def heads_merge():
        return merge_heads([K.retrieve_topk(qh, items, k, normalize_q=False)[:2] for qh in q_heads], k)

    tags = filt = filt_u = None
    if tags_p >= 0:
        tags = (torch.rand(N, generator=g, device=dev) < tags_p).to(torch.int32)
        tags |= torch.randint(0, 1 << 30, (N,), generator=g, device=dev, dtype=torch.int32) << 1  # noise above bit 0
        filt = torch.tensor([[1, 0, 0]], dtype=torch.int32, device=dev).repeat(Q, 1).contiguous()
        if group:
            filt_u = filt[:Q // group].contiguous()

    def fused_tags():
        return K.retrieve_topk(q_bf, items, k, normalize_q=False, tags=tags, tag_filter=filt)

    def fused_excl_tags():
        return K.retrieve_topk(q_bf, items, k, normalize_q=False, exclude_rows=xr, tags=tags, tag_filter=filt)

    def fused_group_tags():
        return K.retrieve_topk_group(q_grp, items, k, normalize_q=False, tags=tags, tag_filter=filt_u)

    extras = []  # (key, function, times): the tagged calls of this run
    if tags is not None:
        extras.append(("tags", fused_tags, []))
        if exclude:
            extras.append(("xtags", fused_excl_tags, []))
        if group:
            extras.append(("gtags", fused_group_tags, []))

    cur = None
    if after:  # page 2 behind the last column of page 1
        p_scores, p_rows, _, _ = fused()
        cur = (p_scores[:, -1].contiguous(), p_rows[:, -1].contiguous())

    def fused_after():
        return K.retrieve_topk(q_bf, items, k, normalize_q=False, after_scores=cur[0], after_rows=cur[1])

    def fused_deep():
        return K.retrieve_topk(q_bf, items, deep, normalize_q=False, deep=True)

    def fused_deep_paged():
        return K.retrieve_topk(q_bf, items, deep, normalize_q=False, deep="paged")

    bias_t = None
    if bias:
        bias_t = (torch.rand(N, generator=g, device=dev) - 0.5) * 0.1

    def fused_bias():
        return K.retrieve_topk(q_bf, items, k, normalize_q=False, bias=bias_t)

    def base(kk=k):
        out = []
        for lo in range(0, Q, BASE_CHUNK):
            out.append((q_bf[lo:lo + BASE_CHUNK] @ items.T).float().topk(kk))
        return out

    def base_deep():
        return base(deep)

    more = []  # (key, function, times, every rep or the baseline's fewer)
    if after:
        more.append(("after", fused_after, [], True))
    if deep:
        more.append(("deep", fused_deep, [], True))
        more.append(("deep_paged", fused_deep_paged, [], True))
        more.append(("deep_base", base_deep, [], False))
    if bias:
        more.append(("bias", fused_bias, [], True))

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    nb = max(3, reps // 4) if name == "evaluation" else reps  # the chunked baseline is long
    for _ in range(2):
        fused()
        if exclude:
            fused_excl()
        if group:
            fused_group()
            heads_merge()
        for _, fn, _ in extras:
            fn()
        for _, fn, _, _ in more:
            fn()
        base()
    torch.cuda.synchronize()
    tf, tx, tb, tg, th = [], [], [], [], []
    for i in range(reps):
        tf.append(timed(fused))
        if exclude:
            tx.append(timed(fused_excl))
        if group:
            tg.append(timed(fused_group))
            th.append(timed(heads_merge))
        for _, fn, times in extras:
            times.append(timed(fn))
        for _, fn, times, every in more:
            if every or i < nb:
                times.append(timed(fn))
        if i < nb:
            tb.append(timed(base))
    scores, rows, _, _ = fused()
    nq = min(Q, 8)
    ref = (q_bf[:nq].float() @ items.float().T).topk(k)
    same = float((rows[:nq].long() == ref.indices).float().mean())
    flop = 2.0 * Q * N * 128
    nbytes = N * 256 + Q * 256 + Q * k * 8
    t_mem, t_mm = nbytes / HBM_PEAK, flop / MFMA_PEAK
    floor_ms = max(t_mem, t_mm) * 1e3
    fm, bm = statistics.median(tf), statistics.median(tb)
    extra = {}
    if exclude:
        # the excluding call's rows against an f32 torch top-k with the lists' rows at -inf
        x_rows = fused_excl()[1]
        sref = q_bf[:nq].float() @ items.float().T
        sref.scatter_(1, xr[:nq].long(), float("-inf"))
        x_same = float((x_rows[:nq].long() == sref.topk(k).indices).float().mean())
        xm = statistics.median(tx)
        extra = {"exclude": exclude, "excl_ms": round(xm, 4), "excl_min_ms": round(min(tx), 4),
                 "excl_max_ms": round(max(tx), 4), "excl_reps": len(tx), "excl_over_fused": round(xm / fm, 4),
                 "excl_over_fused_hi": round(max(tx) / min(tf), 4), "excl_check_rows_equal": round(x_same, 4)}
    if group:
        g_scores, g_rows, _, _ = fused_group()
        m_scores, m_rows = heads_merge()
        g_same = float(((g_rows == m_rows) & (g_scores == m_scores)).float().mean())
        gm, hm = statistics.median(tg), statistics.median(th)
        extra.update({"group": group, "U": Q // group, "group_ms": round(gm, 4), "group_min_ms": round(min(tg), 4),
                      "group_max_ms": round(max(tg), 4), "group_reps": len(tg),
                      "heads_ms": round(hm, 4), "heads_min_ms": round(min(th), 4), "heads_max_ms": round(max(th), 4),
                      "group_over_fused": round(gm / fm, 4), "group_over_fused_hi": round(max(tg) / min(tf), 4),
                      "group_over_heads": round(gm / hm, 4), "group_over_heads_hi": round(max(tg) / min(th), 4),
                      "group_check_rows_equal": round(g_same, 4)})
    if tags is not None:
        t_rows = fused_tags()[1]
        sref = q_bf[:nq].float() @ items.float().T
        sref[:, (tags & 1) == 0] = float("-inf")
        tref = sref.topk(k)
        t_same = float((torch.where(tref.values > float("-inf"), tref.indices, torch.full_like(tref.indices, -1))
                        == t_rows[:nq].long()).float().mean())
        extra.update({"tags_p": tags_p, "tags_eligible": int((tags & 1).sum()), "tags_check_rows_equal": round(t_same, 4)})
        for key, _, times in extras:
            med = statistics.median(times)
            extra.update({f"{key}_ms": round(med, 4), f"{key}_min_ms": round(min(times), 4),
                          f"{key}_max_ms": round(max(times), 4), f"{key}_reps": len(times),
                          f"{key}_over_fused": round(med / fm, 4), f"{key}_over_fused_hi": round(max(times) / min(tf), 4)})
        if group:
            extra.update({"gtags_over_group": round(extra["gtags_ms"] / statistics.median(tg), 4),
                          "gtags_over_group_hi": round(extra["gtags_max_ms"] / min(tg), 4)})
        if exclude:
            extra.update({"xtags_over_excl": round(extra["xtags_ms"] / statistics.median(tx), 4),
                          "xtags_over_excl_hi": round(extra["xtags_max_ms"] / min(tx), 4)})
    stats = {}
    for key, _, times, _ in more:
        stats[key] = statistics.median(times)
        extra.update({f"{key}_ms": round(stats[key], 4), f"{key}_min_ms": round(min(times), 4),
                      f"{key}_max_ms": round(max(times), 4), f"{key}_reps": len(times)})
    if after:
        # page 2 against entries k .. 2k - 1 of an f32 torch top-2k
        a_rows = fused_after()[1]
        ref2 = (q_bf[:nq].float() @ items.float().T).topk(2 * k)
        a_same = float((a_rows[:nq].long() == ref2.indices[:, k:]).float().mean())
        extra.update({"after_over_fused": round(stats["after"] / fm, 4),
                      "after_over_fused_hi": round(extra["after_max_ms"] / min(tf), 4),
                      "after_check_rows_equal": round(a_same, 4)})
    if deep:
        d_scores, d_rows = fused_deep()[:2]
        p_scores, p_rows = fused_deep_paged()[:2]
        d_same = float(((d_rows == p_rows) & (d_scores.view(torch.int32) == p_scores.view(torch.int32))).float().mean())
        refd = (q_bf[:nq].float() @ items.float().T).topk(deep)
        t_same = float((d_rows[:nq].long() == refd.indices).float().mean())
        extra.update({"deep": deep, "deep_passes": len(K.retrieve_deep_passes(deep)),
                      "deep_scan_ms": extra["deep_ms"], "deep_scan_min_ms": extra["deep_min_ms"],
                      "deep_scan_max_ms": extra["deep_max_ms"],
                      "deep_scan_over_paged": round(stats["deep"] / stats["deep_paged"], 4),
                      "deep_scan_over_paged_hi": round(extra["deep_max_ms"] / extra["deep_paged_min_ms"], 4),
                      "deep_over_base": round(stats["deep"] / stats["deep_base"], 4),
                      "deep_over_base_hi": round(extra["deep_max_ms"] / extra["deep_base_min_ms"], 4),
                      "deep_over_fused": round(stats["deep"] / fm, 4), "deep_check_rows_equal": round(d_same, 4),
                      "deep_check_rows_equal_torch": round(t_same, 4)})
    if bias:
        # the biased rows against an f32 torch top-k of scores + bias
        b_rows = fused_bias()[1]
        refb = (q_bf[:nq].float() @ items.float().T + bias_t[None, :]).topk(k)
        b_same = float((b_rows[:nq].long() == refb.indices).float().mean())
        extra.update({"bias_over_fused": round(stats["bias"] / fm, 4),
                      "bias_over_fused_hi": round(extra["bias_max_ms"] / min(tf), 4),
                      "bias_check_rows_equal": round(b_same, 4)})
    print(json.dumps({
        "shape": name, "Q": Q, "N": N, "k": k, "bound": "hbm" if t_mem >= t_mm else "mfma", "floor_ms": round(floor_ms, 4),
        "fused_ms": round(fm, 4), "fused_min_ms": round(min(tf), 4), "fused_max_ms": round(max(tf), 4), "fused_reps": len(tf),
        "fused_floor_frac": round(floor_ms / fm, 4), "fused_tflops": round(flop / fm / 1e9, 1),
        "fused_catalogue_tbps": round(N * 256 / fm / 1e9, 3),
        "base_ms": round(bm, 4), "base_min_ms": round(min(tb), 4), "base_max_ms": round(max(tb), 4), "base_reps": len(tb),
        "base_floor_frac": round(floor_ms / bm, 4), "base_tflops": round(flop / bm / 1e9, 1),
        "speedup": round(bm / fm, 3), "speedup_lo": round(min(tb) / max(tf), 3), "check_rows_equal": round(same, 4),
        **extra,
    }), flush=True)


def child_shards(name: str, N: int, k: int, reps: int, S: int) -> None:
    import torch
    from recommendations_amd import _lib
    from recommendations_amd import kernels as K
    from recommendations_amd.models.lthm.sequence.retrieval import ItemCatalogue
    Q = SHAPES[name]
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    items = torch.empty((N, 128), dtype=torch.bfloat16, device=dev)
    for lo in range(0, N, 1 << 18):
        x = torch.randn((min(1 << 18, N - lo), 128), generator=g, device=dev)
        items[lo:lo + x.shape[0]] = torch.nn.functional.normalize(x, dim=-1).to(torch.bfloat16)
    q_bf = torch.nn.functional.normalize(torch.randn((Q, 128), generator=g, device=dev), dim=-1).to(torch.bfloat16)
    ids = torch.arange(1, N + 1, dtype=torch.int64, device=dev) * 3
    trow = torch.randint(0, N, (Q,), generator=g, device=dev, dtype=torch.int32)
    tid = ids[trow.long()].contiguous()
    has_shards = hasattr(_lib.load(), "lthm_retrieve_merge_shards")
    deep = k > K.RETRIEVE_MAX_K

    def unsharded():
        return K.retrieve_topk(q_bf, items, k, normalize_q=False, target_rows=trow, deep=deep)

    arms = [("unsharded", unsharded, [])]
    if has_shards:
        from recommendations_amd.models.lthm.sequence.retrieval import ShardedItemCatalogue
        full = ItemCatalogue(ids, items)
        parts = full.split(S)
        sh = ShardedItemCatalogue(parts)
        trows = [p.rows_of(tid).contiguous() for p in parts]
        ts = unsharded()[3]
        lists = [K.retrieve_topk(q_bf, p.emb, k, normalize_q=False, target_rows=r, deep=deep, target_scores=ts)
                 for p, r in zip(parts, trows)]
        m_s = torch.stack([x[0] for x in lists])
        m_i = torch.stack([torch.where(x[1] >= 0, p.ids[x[1].clamp(min=0).long()], torch.zeros_like(x[1], dtype=torch.int64))
                           for x, p in zip(lists, parts)])
        m_r = torch.stack([x[2] for x in lists])
        # S full lists of 1,024: descending scores, distinct ids
        d_s = torch.rand((S, Q, 1024), generator=g, device=dev).sort(dim=2, descending=True)[0].contiguous()
        d_i = (torch.arange(S * 1024, device=dev).view(S, 1, 1024) + 1).expand(S, Q, 1024).contiguous()

        def sharded():
            return sh.topk(q_bf, k, normalize_q=False, target_ids=tid)

        def tscore():
            return [K.retrieve_target_score(q_bf, p.emb, r, normalize_q=False) for p, r in zip(parts, trows)]

        def scans():
            return [K.retrieve_topk(q_bf, p.emb, k, normalize_q=False, target_rows=r, deep=deep, target_scores=ts)
                    for p, r in zip(parts, trows)]

        arms += [("sharded", sharded, []), ("tscore", tscore, []), ("scans", scans, []),
                 ("merge", lambda: K.retrieve_merge_shards(m_s, m_i, m_r), []),
                 ("merge_1024", lambda: K.retrieve_merge_shards(d_s, d_i), [])]

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for _ in range(2):
        for _, fn, _ in arms:
            fn()
    torch.cuda.synchronize()
    for _ in range(reps):
        for _, fn, times in arms:
            times.append(timed(fn))
    out = {"shape": name, "mode": "shards", "Q": Q, "N": N, "k": k, "S": S, "reps": reps, "lib": _lib.LIB_PATH}
    med = {}
    for key, _, times in arms:
        med[key] = statistics.median(times)
        out.update({f"{key}_ms": round(med[key], 4), f"{key}_min_ms": round(min(times), 4), f"{key}_max_ms": round(max(times), 4)})
    if has_shards:
        a, b = unsharded(), sharded()
        eq = (torch.equal(b[0], ids[a[1].long()]) and torch.equal(b[1].view(torch.int32), a[0].view(torch.int32))
              and torch.equal(b[2], a[2].long()) and torch.equal(b[3].view(torch.int32), a[3].view(torch.int32)))
        out.update({"sharded_minus_unsharded_ms": round(med["sharded"] - med["unsharded"], 4),
                    "scans_minus_unsharded_ms": round(med["scans"] - med["unsharded"], 4),
                    "merge_floor_ms": round((S + 1) * Q * k * 12 / HBM_PEAK * 1e3, 6),
                    "merge_1024_floor_ms": round((S + 1) * Q * 1024 * 12 / HBM_PEAK * 1e3, 6), "check_equal": bool(eq)})
    print(json.dumps(out), flush=True)


def child_shards_ivf(name: str, N: int, k: int, reps: int, S: int, L: int) -> None:
    """The shards leg: N rows in S id-range shards on one device, L lists per shard, nprobe 1 / 4 / 8 per
    shard.  Arms: the fused call (ShardedClusteredItemCatalogue.topk), the flat sharded scan
    (ShardedItemCatalogue over the same shards) and a Python loop of single-catalogue clustered calls plus
    K.retrieve_merge_shards; recall@k of the clustered list against the flat list."""
    import time
    import torch
    from recommendations_amd import kernels as K
    from recommendations_amd.models.lthm.sequence.retrieval import (ItemCatalogue, ShardedClusteredItemCatalogue,
                                                                    ShardedItemCatalogue)
    Q = SHAPES[name]
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    C, sigma = 4096, 0.7 / 128 ** 0.5
    centres = torch.nn.functional.normalize(torch.randn((C, 128), generator=g, device=dev), dim=-1)
    items = torch.empty((N, 128), dtype=torch.bfloat16, device=dev)
    for lo in range(0, N, 1 << 18):
        n = min(1 << 18, N - lo)
        x = centres[torch.randint(0, C, (n,), generator=g, device=dev)] + sigma * torch.randn((n, 128), generator=g, device=dev)
        items[lo:lo + n] = torch.nn.functional.normalize(x, dim=-1).to(torch.bfloat16)
    xq = centres[torch.randint(0, C, (Q,), generator=g, device=dev)] + sigma * torch.randn((Q, 128), generator=g, device=dev)
    q_bf = torch.nn.functional.normalize(xq, dim=-1).to(torch.bfloat16)
    flat = ItemCatalogue(torch.arange(1, N + 1, dtype=torch.int64, device=dev) * 3, items)
    parts = flat.split(S)
    torch.cuda.synchronize()
    t0 = time.time()
    cl = [p.cluster(L, iters=5, seed=0, sample=min(len(p), 1 << 17)) for p in parts]
    torch.cuda.synchronize()
    build_s = time.time() - t0
    fused, sharded_flat = ShardedClusteredItemCatalogue(cl), ShardedItemCatalogue(parts)
    want = flat.topk(q_bf, k, normalize_q=False)[0]

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), (time.perf_counter() - t) * 1e3

    for P in (1, 4, 8):
        def loop():
            lists = [c.topk(q_bf, k, nprobe=min(P, c.nlist), normalize_q=False) for c in cl]
            return K.retrieve_merge_shards(torch.stack([x[0] for x in lists]), torch.stack([x[1] for x in lists]))

        arms = [("fused", lambda: fused.topk(q_bf, k, nprobe=P, normalize_q=False), []),
                ("sharded_flat", lambda: sharded_flat.topk(q_bf, k, normalize_q=False), []),
                ("loop", loop, [])]
        for _ in range(2):
            for _, fn, _ in arms:
                fn()
        torch.cuda.synchronize()
        for _ in range(reps):
            for _, fn, times in arms:
                times.append(timed(fn))
        out = {"shape": name, "mode": "shards_ivf", "Q": Q, "N": N, "k": k, "S": S, "L": L, "nprobe": P, "reps": reps,
               "build_s": round(build_s, 2)}
        for key, _, times in arms:
            dev_ms, wall_ms = [t[0] for t in times], [t[1] for t in times]
            out.update({f"{key}_ms": round(statistics.median(dev_ms), 4), f"{key}_min_ms": round(min(dev_ms), 4),
                        f"{key}_max_ms": round(max(dev_ms), 4), f"{key}_wall_ms": round(statistics.median(wall_ms), 4)})
        a, b = fused.topk(q_bf, k, nprobe=P, normalize_q=False), loop()
        out["check_equal"] = bool(torch.equal(a[0], b[1]) and torch.equal(a[1].view(torch.int32), b[0].view(torch.int32)))
        hit = (want[:, :, None] == a[0][:, None, :]).any(dim=2).float().sum(dim=1) / k
        out[f"recall_at_{k}"] = round(float(hit.mean()), 4)
        print(json.dumps(out), flush=True)


def child_ivf(name: str, N: int, k: int, reps: int, L: int) -> None:
    import time
    import torch
    from recommendations_amd import _lib
    from recommendations_amd import kernels as K
    from recommendations_amd.models.lthm.sequence.retrieval import ItemCatalogue
    Q = SHAPES[name]
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    C, sigma = 4096, 0.7 / 128 ** 0.5
    centres = torch.nn.functional.normalize(torch.randn((C, 128), generator=g, device=dev), dim=-1)
    items = torch.empty((N, 128), dtype=torch.bfloat16, device=dev)
    for lo in range(0, N, 1 << 18):
        n = min(1 << 18, N - lo)
        x = centres[torch.randint(0, C, (n,), generator=g, device=dev)] + sigma * torch.randn((n, 128), generator=g, device=dev)
        items[lo:lo + n] = torch.nn.functional.normalize(x, dim=-1).to(torch.bfloat16)
    xq = centres[torch.randint(0, C, (Q,), generator=g, device=dev)] + sigma * torch.randn((Q, 128), generator=g, device=dev)
    q_bf = torch.nn.functional.normalize(xq, dim=-1).to(torch.bfloat16)
    flat = ItemCatalogue(torch.arange(1, N + 1, dtype=torch.int64, device=dev) * 3, items)
    torch.cuda.synchronize()
    t0 = time.time()
    cl = flat.cluster(L, iters=5, seed=0, sample=min(N, 1 << 18))
    torch.cuda.synchronize()
    build_s = time.time() - t0
    lens = cl.list_lengths()
    print(json.dumps({"shape": name, "mode": "ivf", "drawn": f"{N} unit rows around {C} random unit centres, noise {sigma:.4f} "
                      "per coordinate; queries drawn the same way", "L": L, "build_s": round(build_s, 2),
                      "list_len_min": int(lens.min()), "list_len_median": int(lens.median()), "list_len_max": int(lens.max())}),
          flush=True)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def flat_call():
        return K.retrieve_topk(q_bf, items, k, normalize_q=False)

    want = flat.topk(q_bf, k, normalize_q=False)[0]
    for P in (1, 8, 32, 64):
        if P > L:
            continue
        probes = cl.probe(q_bf, P, normalize_q=False)
        m_s = torch.rand((P, Q, k), generator=g, device=dev).sort(dim=2, descending=True)[0].contiguous()
        m_i = (torch.arange(P * k, device=dev).view(P, 1, k) + 1).expand(P, Q, k).contiguous()
        arms = [("flat", flat_call, []),
                ("ivf", lambda: cl.topk(q_bf, k, nprobe=P, normalize_q=False), []),
                ("probe", lambda: K.retrieve_topk(q_bf, cl.centroids, P, normalize_q=False), []),
                ("scan_call", lambda: K.retrieve_ivf_topk(q_bf, cl.emb, cl.row_ids, cl.list_off, probes, k, normalize_q=False), []),
                ("merge", lambda: K.retrieve_merge_shards(m_s, m_i), [])]
        for _ in range(2):
            for _, fn, _ in arms:
                fn()
        torch.cuda.synchronize()
        for _ in range(reps):
            for _, fn, times in arms:
                times.append(timed(fn))
        out = {"shape": name, "mode": "ivf", "Q": Q, "N": N, "k": k, "L": L, "nprobe": P, "reps": reps}
        med = {}
        for key, _, times in arms:
            med[key] = statistics.median(times)
            out.update({f"{key}_ms": round(med[key], 4), f"{key}_min_ms": round(min(times), 4), f"{key}_max_ms": round(max(times), 4)})
        out["ivf_over_flat"] = round(med["ivf"] / med["flat"], 4)
        out["ivf_over_flat_hi"] = round(max(arms[1][2]) / min(arms[0][2]), 4)
        parts = {"plan_us": None, "list_scan_us": None, "merge_us": None}
        try:  # device time of the call's own kernels, from one profiled call
            from torch.profiler import ProfilerActivity, profile
            with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
                arms[3][1]()
                torch.cuda.synchronize()
            tot = {"plan_us": 0.0, "list_scan_us": 0.0, "merge_us": 0.0}
            for ev in prof.events():
                dt = float(ev.device_time if hasattr(ev, "device_time") else getattr(ev, "cuda_time", 0.0))
                if "retr_ivf_topk_k" in ev.name:
                    tot["list_scan_us"] += dt
                elif "retr_ivf_" in ev.name:
                    tot["plan_us"] += dt
                elif "retr_shard_merge_k" in ev.name:
                    tot["merge_us"] += dt
            if tot["list_scan_us"] > 0:
                parts = {key: round(v, 1) for key, v in tot.items()}
        except Exception as e:  # the timings above stand without it
            parts["profile_error"] = repr(e)[:200]
        out.update(parts)
        got = cl.topk(q_bf, k, nprobe=P, normalize_q=False)[1]
        hit = (want[:, :, None] == got[:, None, :]).any(dim=2).float().sum(dim=1) / k
        out[f"recall_at_{k}"] = round(float(hit.mean()), 4)
        out["rows_per_query"] = round(float(lens[probes.long()].sum(dim=1).float().mean()), 1)
        print(json.dumps(out), flush=True)


def child_ivf_heads(name: str, N: int, k: int, reps: int, L: int, G: int) -> None:
    """--ivf-heads: child_ivf's catalogue, U users of G queries each, every query drawn around a centre of
    its own (the heads of a user point at different lists: the hard case for one shared probe row)."""
    import torch
    from recommendations_amd import kernels as K
    from recommendations_amd.models.lthm.sequence.retrieval import ItemCatalogue
    U = SHAPES[name]
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    C, sigma = 4096, 0.7 / 128 ** 0.5  # child_ivf's catalogue, drawn the same way
    centres = torch.nn.functional.normalize(torch.randn((C, 128), generator=g, device=dev), dim=-1)
    items = torch.empty((N, 128), dtype=torch.bfloat16, device=dev)
    for lo in range(0, N, 1 << 18):
        n = min(1 << 18, N - lo)
        x = centres[torch.randint(0, C, (n,), generator=g, device=dev)] + sigma * torch.randn((n, 128), generator=g, device=dev)
        items[lo:lo + n] = torch.nn.functional.normalize(x, dim=-1).to(torch.bfloat16)
    xq = centres[torch.randint(0, C, (U * G,), generator=g, device=dev)] + sigma * torch.randn((U * G, 128), generator=g, device=dev)
    q = torch.nn.functional.normalize(xq, dim=-1).to(torch.bfloat16).view(U, G, 128).contiguous()
    heads = [q[:, i].contiguous() for i in range(G)]
    flat = ItemCatalogue(torch.arange(1, N + 1, dtype=torch.int64, device=dev) * 3, items)
    cl = flat.cluster(L, iters=5, seed=0, sample=min(N, 1 << 18))
    view = cl.with_heads()
    lens = cl.list_lengths()
    P = 8

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def separate():
        return merge_heads([cl.topk(h, k, nprobe=P, normalize_q=False) for h in heads], k)

    arms = [("ivf_heads", lambda: view.topk(q, k, nprobe=P, normalize_q=False), []),
            ("flat_group", lambda: K.retrieve_topk_group(q, items, k, normalize_q=False), []),
            ("separate", separate, [])]
    for _ in range(2):
        for _, fn, _ in arms:
            fn()
    torch.cuda.synchronize()
    for _ in range(reps):
        for _, fn, times in arms:
            times.append(timed(fn))
    out = {"shape": name, "mode": "ivf_heads", "U": U, "G": G, "N": N, "k": k, "L": L, "nprobe": P, "reps": reps,
           "heads": "every query around a centre of its own"}
    for key, _, times in arms:
        out.update({f"{key}_ms": round(statistics.median(times), 4), f"{key}_min_ms": round(min(times), 4),
                    f"{key}_max_ms": round(max(times), 4)})
    out["heads_over_flat"] = round(out["ivf_heads_ms"] / out["flat_group_ms"], 4)
    out["heads_over_flat_hi"] = round(out["ivf_heads_max_ms"] / out["flat_group_min_ms"], 4)  # the worst pairing
    out["heads_over_separate"] = round(out["ivf_heads_ms"] / out["separate_ms"], 4)
    want = flat.topk(q, k, normalize_q=False)[0]

    def recall(got):
        return round(float(((want[:, :, None] == got[:, None, :]).any(dim=2).float().sum(dim=1) / k).mean()), 4)

    got = view.topk(q, k, nprobe=P, normalize_q=False)[1]
    out[f"recall_at_{k}"] = recall(got)
    out[f"separate_recall_at_{k}"] = recall(separate()[1])
    out["no_item_twice"] = bool((got.sort(dim=1)[0][:, 1:] != got.sort(dim=1)[0][:, :-1]).logical_or(got.sort(dim=1)[0][:, 1:] == 0).all())
    out["rows_per_user"] = round(float(lens[view.probe(q, P, normalize_q=False).long()].sum(dim=1).float().mean()), 1)
    out["separate_rows_per_user"] = round(float(sum(lens[cl.probe(h, P, normalize_q=False).long()].sum(dim=1).float().mean()
                                                    for h in heads)), 1)
    print(json.dumps(out), flush=True)


def child_ivf_filt(name: str, N: int, k: int, reps: int, L: int, baseline_lib: str) -> None:
    import ctypes
    import torch
    from recommendations_amd import _lib
    from recommendations_amd import kernels as K
    from recommendations_amd._lib import dcode, ptr, stream
    from recommendations_amd.models.lthm.sequence.retrieval import ItemCatalogue
    Q = SHAPES[name]
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    C, sigma = 4096, 0.7 / 128 ** 0.5  # child_ivf's catalogue and queries, drawn the same way
    centres = torch.nn.functional.normalize(torch.randn((C, 128), generator=g, device=dev), dim=-1)
    items = torch.empty((N, 128), dtype=torch.bfloat16, device=dev)
    for lo in range(0, N, 1 << 18):
        n = min(1 << 18, N - lo)
        x = centres[torch.randint(0, C, (n,), generator=g, device=dev)] + sigma * torch.randn((n, 128), generator=g, device=dev)
        items[lo:lo + n] = torch.nn.functional.normalize(x, dim=-1).to(torch.bfloat16)
    xq = centres[torch.randint(0, C, (Q,), generator=g, device=dev)] + sigma * torch.randn((Q, 128), generator=g, device=dev)
    q_bf = torch.nn.functional.normalize(xq, dim=-1).to(torch.bfloat16)
    tags = torch.randint(0, 2, (N,), generator=g, device=dev).to(torch.int32)
    bias = (0.05 * torch.randn((N,), generator=g, device=dev)).contiguous()
    flat = ItemCatalogue(torch.arange(1, N + 1, dtype=torch.int64, device=dev) * 3, items, tags, bias)
    cl = flat.cluster(L, iters=5, seed=0, sample=min(N, 1 << 18))
    view = cl.with_filters()
    flat = cl.to_flat()
    torch.cuda.synchronize()
    zero_f = torch.zeros((Q, 3), dtype=torch.int32, device=dev)
    half_f = torch.tensor([[1, 0, 0]] * Q, dtype=torch.int32, device=dev)
    zero_w = torch.zeros(Q, dtype=torch.float32, device=dev)
    one_w = torch.ones(Q, dtype=torch.float32, device=dev)
    base = ctypes.CDLL(baseline_lib) if baseline_lib else None  # RTLD_LOCAL: its own kernels behind its own entry
    if base is not None:
        base.lthm_retrieve_ivf_topk.restype = ctypes.c_int
        base.lthm_retrieve_ivf_topk.argtypes = _lib.load().lthm_retrieve_ivf_topk.argtypes

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for P in (1, 8, 32):
        if P > L:
            continue
        probes = cl.probe(q_bf, P, normalize_q=False)
        need = _lib.load().lthm_retrieve_ivf_ws_bytes(Q, N, L, P, k, 0)
        sc = torch.empty((Q, k), dtype=torch.float32, device=dev)
        ids = torch.empty((Q, k), dtype=torch.int64, device=dev)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)

        def scan_call(lib):
            rc = lib.lthm_retrieve_ivf_topk(ptr(cl.emb), N, ptr(cl.row_ids), ptr(cl.list_off), L, ptr(q_bf), dcode(q_bf), 0, Q,
                                            ptr(probes), P, k, None, ptr(sc), ptr(ids), ptr(ws), need, stream())
            if rc != 0:
                raise RuntimeError(f"lthm_retrieve_ivf_topk failed with hip error {rc}")

        arms = [("plain", lambda: cl.topk(q_bf, k, nprobe=P, normalize_q=False), []),
                ("neutral", lambda: view.topk(q_bf, k, nprobe=P, normalize_q=False, tag_filter=zero_f, bias_weight=zero_w), []),
                ("filt", lambda: view.topk(q_bf, k, nprobe=P, normalize_q=False, tag_filter=half_f, bias_weight=one_w), []),
                ("flat", lambda: flat.topk(q_bf, k, normalize_q=False, tag_filter=half_f, bias_weight=one_w), [])]
        if base is not None:
            arms += [("base_scan_call", lambda: scan_call(base), []), ("scan_call", lambda: scan_call(_lib.load()), [])]
        for _ in range(2):
            for _, fn, _ in arms:
                fn()
        torch.cuda.synchronize()
        for _ in range(reps):
            for _, fn, times in arms:
                times.append(timed(fn))
        out = {"shape": name, "mode": "ivf_filt", "Q": Q, "N": N, "k": k, "L": L, "nprobe": P, "reps": reps}
        med, lo_, hi_ = {}, {}, {}
        for key, _, times in arms:
            med[key], lo_[key], hi_[key] = statistics.median(times), min(times), max(times)
            out.update({f"{key}_ms": round(med[key], 4), f"{key}_min_ms": round(lo_[key], 4), f"{key}_max_ms": round(hi_[key], 4)})
        for a, b in (("neutral", "plain"), ("filt", "plain"), ("filt", "flat")) + ((("scan_call", "base_scan_call"),) if base else ()):
            tag = "scan_call_over_base" if b == "base_scan_call" else f"{a}_over_{b}"
            out[tag] = round(med[a] / med[b], 4)
            out[tag + "_hi"] = round(hi_[a] / lo_[b], 4)
        p_s, p_i = cl.topk(q_bf, k, nprobe=P, normalize_q=False)
        n_s, n_i = view.topk(q_bf, k, nprobe=P, normalize_q=False, tag_filter=zero_f, bias_weight=zero_w)
        out["neutral_equals_plain"] = bool(torch.equal(p_i, n_i) and torch.equal(p_s.view(torch.int32), n_s.view(torch.int32)))
        # the flat list's entries that lie in a probed list are, in order, the head of the clustered list
        f_s, f_i = view.topk(q_bf, k, nprobe=P, normalize_q=False, tag_filter=half_f, bias_weight=one_w)
        w_i, w_s, _, _ = flat.topk(q_bf, k, normalize_q=False, tag_filter=half_f, bias_weight=one_w)
        lists = torch.bucketize(cl.rows_of(w_i).long().clamp(min=0), cl.list_off[1:], right=True)
        probed = (lists[:, :, None] == probes.long()[:, None, :]).any(dim=2) & (w_i != 0)
        ok = True
        for i in range(min(Q, 64)):
            m = int(probed[i].sum())
            ok = ok and torch.equal(w_i[i][probed[i]], f_i[i, :m]) and torch.equal(w_s[i][probed[i]], f_s[i, :m])
        out["filt_equals_flat_on_probed"] = bool(ok)
        hit = ((w_i[:, :, None] == f_i[:, None, :]).any(dim=2) & (w_i != 0)).float().sum(dim=1) / (w_i != 0).sum(dim=1).clamp(min=1)
        out[f"filt_recall_at_{k}"] = round(float(hit.mean()), 4)
        print(json.dumps(out), flush=True)


def child_ivf_deep(name: str, N: int, reps: int, L: int, baseline_lib: str) -> None:
    import ctypes
    import torch
    from recommendations_amd import _lib
    from recommendations_amd._lib import dcode, ptr, stream
    from recommendations_amd.models.lthm.sequence.retrieval import ItemCatalogue
    Q = SHAPES[name]
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    C, sigma = 4096, 0.7 / 128 ** 0.5  # child_ivf's catalogue and queries, drawn the same way
    centres = torch.nn.functional.normalize(torch.randn((C, 128), generator=g, device=dev), dim=-1)
    items = torch.empty((N, 128), dtype=torch.bfloat16, device=dev)
    for lo in range(0, N, 1 << 18):
        n = min(1 << 18, N - lo)
        x = centres[torch.randint(0, C, (n,), generator=g, device=dev)] + sigma * torch.randn((n, 128), generator=g, device=dev)
        items[lo:lo + n] = torch.nn.functional.normalize(x, dim=-1).to(torch.bfloat16)
    xq = centres[torch.randint(0, C, (Q,), generator=g, device=dev)] + sigma * torch.randn((Q, 128), generator=g, device=dev)
    q_bf = torch.nn.functional.normalize(xq, dim=-1).to(torch.bfloat16)
    groups = torch.randint(0, 64, (N,), generator=g, device=dev).to(torch.int32)
    flat = ItemCatalogue(torch.arange(1, N + 1, dtype=torch.int64, device=dev) * 3, items, groups=groups)
    cl = flat.cluster(L, iters=5, seed=0, sample=min(N, 1 << 18))
    view = cl.with_deep(groups)
    torch.cuda.synchronize()
    base = ctypes.CDLL(baseline_lib) if baseline_lib else None  # RTLD_LOCAL: its own kernels behind its own entry
    if base is not None:
        base.lthm_retrieve_ivf_topk.restype = ctypes.c_int
        base.lthm_retrieve_ivf_topk.argtypes = _lib.load().lthm_retrieve_ivf_topk.argtypes

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def run(arms, out):
        for _ in range(2):
            for _, fn, _ in arms:
                fn()
        torch.cuda.synchronize()
        for _ in range(reps):
            for _, fn, times in arms:  # all arms alternate in one loop
                times.append(timed(fn))
        for key, _, times in arms:
            out.update({f"{key}_ms": round(statistics.median(times), 4), f"{key}_min_ms": round(min(times), 4),
                        f"{key}_max_ms": round(max(times), 4)})

    for P in (8, 32):
        if P > L:
            continue
        probes = cl.probe(q_bf, P, normalize_q=False)
        k0 = 100
        need = _lib.load().lthm_retrieve_ivf_ws_bytes(Q, N, L, P, k0, 0)
        sc = torch.empty((Q, k0), dtype=torch.float32, device=dev)
        ids = torch.empty((Q, k0), dtype=torch.int64, device=dev)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)

        def scan_call(lib):
            rc = lib.lthm_retrieve_ivf_topk(ptr(cl.emb), N, ptr(cl.row_ids), ptr(cl.list_off), L, ptr(q_bf), dcode(q_bf), 0, Q,
                                            ptr(probes), P, k0, None, ptr(sc), ptr(ids), ptr(ws), need, stream())
            if rc != 0:
                raise RuntimeError(f"lthm_retrieve_ivf_topk failed with hip error {rc}")

        for k in (256, 1024):
            out = {"shape": name, "mode": "ivf_deep", "Q": Q, "N": N, "k": k, "L": L, "nprobe": P, "reps": reps}
            arms = [("ivf_deep", lambda: view.topk(q_bf, k, nprobe=P, normalize_q=False), []),
                    ("flat_deep", lambda: flat.topk(q_bf, k, normalize_q=False), [])]
            if base is not None:
                arms += [("base_scan_call", lambda: scan_call(base), []), ("scan_call", lambda: scan_call(_lib.load()), [])]
            run(arms, out)
            out["deep_over_flat"] = round(out["ivf_deep_ms"] / out["flat_deep_ms"], 4)
            out["deep_over_flat_hi"] = round(out["ivf_deep_max_ms"] / out["flat_deep_min_ms"], 4)  # the worst pairing
            if base is not None:  # the existing k = 100 path did not move: each median inside the other's range
                out["scan_call_within_base"] = bool(out["base_scan_call_min_ms"] <= out["scan_call_ms"] <= out["base_scan_call_max_ms"]
                                                    and out["scan_call_min_ms"] <= out["base_scan_call_ms"] <= out["scan_call_max_ms"])
            # the flat list's entries that lie in a probed list are, in order, the head of the clustered list
            f_s, f_i = view.topk(q_bf, k, nprobe=P, normalize_q=False)
            w_i, w_s, _, _ = flat.topk(q_bf, k, normalize_q=False)
            lists = torch.bucketize(cl.rows_of(w_i).long().clamp(min=0), cl.list_off[1:], right=True)
            ok, hits = True, 0.0
            for i in range(0, Q, 64):
                probed = (lists[i:i + 64, :, None] == probes.long()[i:i + 64, None, :]).any(dim=2) & (w_i[i:i + 64] != 0)
                hits += float(probed.float().sum(dim=1).div((w_i[i:i + 64] != 0).sum(dim=1).clamp(min=1)).sum())
                for j in range(probed.shape[0] if i == 0 else 0):
                    m = int(probed[j].sum())
                    ok = ok and torch.equal(w_i[j][probed[j]], f_i[j, :m]) \
                        and torch.equal(w_s[j][probed[j]].view(torch.int32), f_s[j, :m].view(torch.int32))
            out["deep_equals_flat_on_probed"] = bool(ok)
            out[f"recall_at_{k}"] = round(hits / Q, 4)  # a flat entry in a probed list is in the clustered list: checked above
            print(json.dumps(out), flush=True)
        if name == "serving":  # the wrapper-level chain: deep pool 1,024 -> diversify k = 100, clustered against flat
            out = {"shape": name, "mode": "ivf_deep_diversify", "Q": Q, "N": N, "pool": 1024, "k": 100, "L": L, "nprobe": P,
                   "reps": reps}

            def chain_ivf():
                s, i = view.topk(q_bf, 1024, nprobe=P, normalize_q=False)
                return view.diversify(i, s, 100, lam=0.7, group_cap=2)

            def chain_flat():
                i, s, _, _ = flat.topk(q_bf, 1024, normalize_q=False)
                return flat.diversify(i, s, 100, lam=0.7, group_cap=2)

            run([("ivf_chain", chain_ivf, []), ("flat_chain", chain_flat, [])], out)
            out["chain_over_flat"] = round(out["ivf_chain_ms"] / out["flat_chain_ms"], 4)
            out["chain_over_flat_hi"] = round(out["ivf_chain_max_ms"] / out["flat_chain_min_ms"], 4)
            print(json.dumps(out), flush=True)


def child_diversify(N: int, k: int, reps: int) -> None:
    import torch
    from recommendations_amd import kernels as K
    Q, lam_v = 256, 0.7
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    C, sigma = 4096, 0.7 / 128 ** 0.5
    centres = torch.nn.functional.normalize(torch.randn((C, 128), generator=g, device=dev), dim=-1)
    items = torch.empty((N, 128), dtype=torch.bfloat16, device=dev)
    for lo in range(0, N, 1 << 18):
        n = min(1 << 18, N - lo)
        x = centres[torch.randint(0, C, (n,), generator=g, device=dev)] + sigma * torch.randn((n, 128), generator=g, device=dev)
        items[lo:lo + n] = torch.nn.functional.normalize(x, dim=-1).to(torch.bfloat16)
    xq = centres[torch.randint(0, C, (Q,), generator=g, device=dev)] + sigma * torch.randn((Q, 128), generator=g, device=dev)
    q_bf = torch.nn.functional.normalize(xq, dim=-1).to(torch.bfloat16)
    lam = torch.full((Q,), lam_v, dtype=torch.float32, device=dev)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for M in (512, 1024):
        sc, rw, _, _ = K.retrieve_topk(q_bf, items, M, normalize_q=False, deep=True)
        sc, rw = sc.contiguous(), rw.contiguous()

        def torch_greedy():
            X = items[rw.long()].float()  # [Q, M, 128]: the gather is part of the baseline, as it is of the kernel
            d = torch.zeros_like(sc)
            taken = torch.zeros_like(sc, dtype=torch.bool)
            out = torch.empty((Q, k), dtype=torch.int64, device=dev)
            ar = torch.arange(Q, device=dev)
            for t in range(k):
                m = (lam_v * sc - (1.0 - lam_v) * d).masked_fill(taken, float("-inf"))
                j = m.argmax(dim=1)
                out[:, t] = j
                taken[ar, j] = True
                d = torch.maximum(d, torch.bmm(X, X[ar, j][:, :, None])[:, :, 0])
            return rw.gather(1, out)

        arms = [("kernel", lambda: K.retrieve_diversify(items, rw, sc, k, lam=lam), []), ("torch", torch_greedy, [])]
        for _ in range(2):
            for _, fn, _ in arms:
                fn()
        torch.cuda.synchronize()
        for _ in range(reps):
            for _, fn, times in arms:
                times.append(timed(fn))
        out = {"mode": "diversify", "Q": Q, "N": N, "M": M, "k": k, "lam": lam_v, "reps": reps}
        med = {}
        for key, _, times in arms:
            med[key] = statistics.median(times)
            out.update({f"{key}_ms": round(med[key], 4), f"{key}_min_ms": round(min(times), 4), f"{key}_max_ms": round(max(times), 4)})
        out["kernel_over_torch"] = round(med["kernel"] / med["torch"], 4)
        out["kernel_over_torch_hi"] = round(max(arms[0][2]) / min(arms[1][2]), 4)
        out["fma_per_s"] = round(Q * k * M * 128 / (med["kernel"] * 1e-3), 0)
        out["same_rows"] = round(float((arms[0][1]()[0].long() == torch_greedy()).float().mean()), 4)
        print(json.dumps(out), flush=True)


def child_q8(name: str, N: int, k: int, reps: int, pool: int) -> None:
    """The e4m3 catalogue against the bf16 one, all arms alternating in one loop: the flat deep scan at
    k = pool (the bf16 way to such a shortlist), the e4m3 scan at pool, the e4m3 scan plus the re-scoring to
    k, the flat call at k, and the torch baseline."""
    import torch
    from recommendations_amd import kernels as K
    Q = SHAPES[name]
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    C, sigma = 4096, 0.7 / 128 ** 0.5
    centres = torch.nn.functional.normalize(torch.randn((C, 128), generator=g, device=dev), dim=-1)
    items = torch.empty((N, 128), dtype=torch.bfloat16, device=dev)
    for lo in range(0, N, 1 << 18):
        n = min(1 << 18, N - lo)
        x = centres[torch.randint(0, C, (n,), generator=g, device=dev)] + sigma * torch.randn((n, 128), generator=g, device=dev)
        items[lo:lo + n] = torch.nn.functional.normalize(x, dim=-1).to(torch.bfloat16)
    xq = centres[torch.randint(0, C, (Q,), generator=g, device=dev)] + sigma * torch.randn((Q, 128), generator=g, device=dev)
    q_bf = torch.nn.functional.normalize(xq, dim=-1).to(torch.bfloat16)
    codes, scale = K.quantize_catalogue_q8(items)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def two_stage():
        rows = K.retrieve_q8_topk(q_bf, codes, scale, pool, normalize_q=False)[1]
        return K.retrieve_rescore(q_bf, items, rows, k, normalize_q=False)

    def base():
        return [(q_bf[lo:lo + BASE_CHUNK] @ items.T).float().topk(k) for lo in range(0, Q, BASE_CHUNK)]

    arms = [("flat_deep", lambda: K.retrieve_topk(q_bf, items, pool, normalize_q=False, deep=True), []),
            ("q8_scan", lambda: K.retrieve_q8_topk(q_bf, codes, scale, pool, normalize_q=False), []),
            ("q8_two_stage", two_stage, []),
            ("flat", lambda: K.retrieve_topk(q_bf, items, k, normalize_q=False), []),
            ("torch", base, [])]
    for _ in range(2):
        for _, fn, _ in arms:
            fn()
    torch.cuda.synchronize()
    for _ in range(reps):
        for _, fn, times in arms:
            times.append(timed(fn))
    out = {"shape": name, "mode": "q8", "Q": Q, "N": N, "k": k, "pool": pool, "reps": reps,
           "drawn": f"{N} unit rows around {C} random unit centres, noise {sigma:.4f} per coordinate; queries drawn the same way",
           "bf16_bytes_per_scan": N * 256, "q8_bytes_per_scan": N * 132}
    med = {}
    for key, _, times in arms:
        med[key] = statistics.median(times)
        out.update({f"{key}_ms": round(med[key], 4), f"{key}_min_ms": round(min(times), 4), f"{key}_max_ms": round(max(times), 4)})
    out["q8_scan_over_flat_deep"] = round(med["q8_scan"] / med["flat_deep"], 4)
    out["q8_two_stage_over_flat"] = round(med["q8_two_stage"] / med["flat"], 4)
    want = K.retrieve_topk(q_bf, items, k, normalize_q=False)[1]
    got = two_stage()[1]
    hit = ((want[:, :, None] == got[:, None, :]).any(dim=2) & (want >= 0)[:, :, None].any(dim=2)).float().sum(dim=1) / k
    out[f"recall_at_{k}"] = round(float(hit.mean()), 4)
    out[f"recall_at_{k}_min"] = round(float(hit.min()), 4)
    print(json.dumps(out), flush=True)


def child_ivf_q8(name: str, N: int, reps: int, L: int) -> None:
    """The clustered e4m3 catalogue against its bf16 twin on --ivf's catalogue with a 50 %-selective tag
    filter and a prior, nprobe 8, one line per pool in {256, 1024}, all arms alternating in one loop:
    (a) the bf16 with_deep() call at k = pool, (b) the e4m3 scan at pool, (c) the e4m3 scan plus the
    re-scoring to k = 100, (d) the bf16 with_filters() call at k = 100."""
    import torch
    from recommendations_amd.models.lthm.sequence.retrieval import ItemCatalogue
    Q = SHAPES[name]
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    C, sigma = 4096, 0.7 / 128 ** 0.5  # child_ivf's catalogue and queries, drawn the same way
    centres = torch.nn.functional.normalize(torch.randn((C, 128), generator=g, device=dev), dim=-1)
    items = torch.empty((N, 128), dtype=torch.bfloat16, device=dev)
    for lo in range(0, N, 1 << 18):
        n = min(1 << 18, N - lo)
        x = centres[torch.randint(0, C, (n,), generator=g, device=dev)] + sigma * torch.randn((n, 128), generator=g, device=dev)
        items[lo:lo + n] = torch.nn.functional.normalize(x, dim=-1).to(torch.bfloat16)
    xq = centres[torch.randint(0, C, (Q,), generator=g, device=dev)] + sigma * torch.randn((Q, 128), generator=g, device=dev)
    q_bf = torch.nn.functional.normalize(xq, dim=-1).to(torch.bfloat16)
    tags = torch.randint(0, 2, (N,), generator=g, device=dev).to(torch.int32)  # bit 0 on half the rows
    bias = (0.05 * torch.randn((N,), generator=g, device=dev)).contiguous()
    flat = ItemCatalogue(torch.arange(1, N + 1, dtype=torch.int64, device=dev) * 3, items, tags=tags, bias=bias)
    cl = flat.cluster(L, iters=5, seed=0, sample=min(N, 1 << 18))
    deep, filt_view, qc = cl.with_deep(), cl.with_filters(), cl.quantize()
    from recommendations_amd.models.lthm.sequence.retrieval import make_tag_filter
    filt = make_tag_filter(Q, tag_all=1, device=dev)
    P, k, w = 8, 100, 1.0
    torch.cuda.synchronize()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for pool in (256, 1024):
        kw = dict(nprobe=P, normalize_q=False, tag_filter=filt, bias_weight=w)
        arms = [("bf16_deep", lambda: deep.topk(q_bf, pool, **kw), []),
                ("q8_scan", lambda: qc.topk(q_bf, pool, shortlist=pool, rescore=False, **kw), []),
                ("q8_two_stage", lambda: qc.topk(q_bf, k, shortlist=pool, **kw), []),
                ("bf16_filt", lambda: filt_view.topk(q_bf, k, **kw), [])]
        for _ in range(2):
            for _, fn, _ in arms:
                fn()
        torch.cuda.synchronize()
        for _ in range(reps):
            for _, fn, times in arms:
                times.append(timed(fn))
        lens = cl.list_lengths()
        out = {"shape": name, "mode": "ivf_q8", "Q": Q, "N": N, "L": L, "nprobe": P, "pool": pool, "k": k, "reps": reps,
               "tag_selectivity": round(float((tags & 1).float().mean()), 4), "bias_weight": w,
               "list_len_median": int(lens.median()), "list_len_max": int(lens.max()),
               "bytes_per_row_bf16": 256 + 8 + 4 + 4, "bytes_per_row_q8": 132 + 8 + 4 + 4,
               "bytes_per_row_q8_keep_exact": 132 + 256 + 8 + 4 + 4}
        med = {}
        for key, _, times in arms:
            med[key] = statistics.median(times)
            out.update({f"{key}_ms": round(med[key], 4), f"{key}_min_ms": round(min(times), 4), f"{key}_max_ms": round(max(times), 4)})
        out["q8_scan_over_bf16_deep"] = round(med["q8_scan"] / med["bf16_deep"], 4)
        out["q8_scan_over_bf16_deep_hi"] = round(out["q8_scan_max_ms"] / out["bf16_deep_min_ms"], 4)  # the worst pairing
        out["q8_two_stage_over_bf16_filt"] = round(med["q8_two_stage"] / med["bf16_filt"], 4)
        out["q8_two_stage_over_bf16_filt_hi"] = round(out["q8_two_stage_max_ms"] / out["bf16_filt_min_ms"], 4)
        out[f"recall_at_{k}"] = round(qc.recall(q_bf, k, P, pool, tag_filter=filt, bias_weight=w), 4)
        print(json.dumps(out), flush=True)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="serving,evaluation")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--n-items", type=int, default=2_000_000)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--exclude", type=int, default=0,
                    help="also time the call with X random excluded rows per query (1..1024), in the same loop")
    ap.add_argument("--group", type=int, default=0,
                    help="also time the grouped call with G queries per user (2..8), the G plain calls and their merge")
    ap.add_argument("--tags", type=float, default=-1.0,
                    help="also time the filtered call with random tags, a fraction P (0..1) of the rows eligible")
    ap.add_argument("--after", action="store_true",
                    help="also time page 2 (the k rows behind page 1's last column) next to page 1, in the same loop")
    ap.add_argument("--deep", type=int, default=0,
                    help="also time the deep list of K rows (129..1024), single-scan and paged, against the torch baseline's top-K")
    ap.add_argument("--bias", action="store_true",
                    help="also time the call with a random f32 bias per row and weight 1 next to the plain call")
    ap.add_argument("--shards", type=int, default=0,
                    help="a mode of its own: the catalogue as S shards (1..64) on this device against the unsharded call")
    ap.add_argument("--shards-ivf", type=int, default=0,
                    help="with --shards S: S clustered shards of this many lists each (the sharded clustered call "
                         "against the flat sharded scan and a Python loop of clustered calls)")
    ap.add_argument("--ivf", type=int, default=0,
                    help="a mode of its own: the catalogue clustered into L lists, nprobe in {1, 8, 32, 64}, against the flat call")
    ap.add_argument("--ivf-filt", type=int, default=0,
                    help="a mode of its own: --ivf's catalogue with tags and a bias, the with_filters() view against "
                         "the plain clustered call and the flat call, nprobe in {1, 8, 32}")
    ap.add_argument("--ivf-deep", type=int, default=0,
                    help="a mode of its own: --ivf's catalogue, the with_deep() view's k = 256 / 1,024 lists against the "
                         "flat deep call, and the chain deep pool -> diversify")
    ap.add_argument("--ivf-heads", type=int, default=0,
                    help="a mode of its own: --ivf's catalogue, --group (default 3) queries per user, nprobe 8: the "
                         "with_heads() view against the flat grouped call and against one clustered call per head")
    ap.add_argument("--baseline-lib", default="",
                    help="with --ivf-filt / --ivf-deep: another build of liblthm_hip.so whose lthm_retrieve_ivf_topk is timed "
                         "in the same loop")
    ap.add_argument("--diversify", action="store_true",
                    help="a mode of its own: K.retrieve_diversify on pools of 512 and 1,024 against a torch greedy loop")
    ap.add_argument("--q8", type=int, default=0,
                    help="a mode of its own: the e4m3 scan at POOL (1..1024) and the two-stage list against the flat calls")
    ap.add_argument("--ivf-q8", type=int, default=0,
                    help="a mode of its own: --ivf's catalogue with tags and a bias, quantised (ClusteredItemCatalogue.quantize): "
                         "the e4m3 scan at pools 256 / 1,024 and the two-stage list against the with_deep() / with_filters() calls")
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if not 0 <= a.exclude <= 1024:
        raise SystemExit("--exclude takes 0 (off) or 1..1024 rows per query")
    if a.group and not 2 <= a.group <= 8:
        raise SystemExit("--group takes 0 (off) or 2..8 queries per user")
    if a.tags != -1.0 and not 0.0 <= a.tags <= 1.0:
        raise SystemExit("--tags takes a fraction in 0..1")
    if a.deep and not 129 <= a.deep <= 1024:
        raise SystemExit("--deep takes 0 (off) or a list length in 129..1024")
    if not 0 <= a.shards <= 64:
        raise SystemExit("--shards takes 0 (off) or 1..64 shards")
    if a.ivf < 0 or (a.ivf and a.shards):
        raise SystemExit("--ivf takes 0 (off) or a number of lists, and is a mode of its own")
    if a.diversify and (a.ivf or a.shards or not 1 <= a.k <= 128):
        raise SystemExit("--diversify is a mode of its own and takes --k in 1..128")
    if not 0 <= a.q8 <= 1024 or (a.q8 and (a.ivf or a.shards or a.diversify or not 1 <= a.k <= min(a.q8, 128))):
        raise SystemExit("--q8 takes 0 (off) or a pool of 1..1024, is a mode of its own and takes --k in 1..min(pool, 128)")
    if a.ivf_filt < 0 or (a.ivf_filt and (a.ivf or a.shards or a.diversify or a.q8 or not 1 <= a.k <= 128)):
        raise SystemExit("--ivf-filt takes 0 (off) or a number of lists, is a mode of its own and takes --k in 1..128")
    if a.ivf_deep < 0 or (a.ivf_deep and (a.ivf or a.ivf_filt or a.shards or a.diversify or a.q8)):
        raise SystemExit("--ivf-deep takes 0 (off) or a number of lists, and is a mode of its own")
    if a.baseline_lib and not ((a.ivf_filt or a.ivf_deep) and os.path.exists(a.baseline_lib)):
        raise SystemExit("--baseline-lib takes the path of a built liblthm_hip.so and goes with --ivf-filt or --ivf-deep")
    if a.ivf_heads < 0 or (a.ivf_heads and (a.ivf or a.ivf_filt or a.ivf_deep or a.shards or a.diversify or a.q8
                                            or not 1 <= a.k <= 128)):
        raise SystemExit("--ivf-heads takes 0 (off) or a number of lists, is a mode of its own and takes --k in 1..128")
    if a.ivf_q8 < 0 or (a.ivf_q8 and (a.ivf or a.ivf_filt or a.ivf_deep or a.ivf_heads or a.shards or a.diversify or a.q8)):
        raise SystemExit("--ivf-q8 takes 0 (off) or a number of lists, and is a mode of its own")
    if a.child and a.ivf_q8:
        child_ivf_q8(a.child, a.n_items, a.reps, a.ivf_q8)
        return 0
    if a.child and a.ivf_heads:
        child_ivf_heads(a.child, a.n_items, a.k, a.reps, a.ivf_heads, a.group or 3)
        return 0
    if a.child and a.ivf_deep:
        child_ivf_deep(a.child, a.n_items, a.reps, a.ivf_deep, a.baseline_lib)
        return 0
    if a.child and a.ivf_filt:
        child_ivf_filt(a.child, a.n_items, a.k, a.reps, a.ivf_filt, a.baseline_lib)
        return 0
    if a.child and a.q8:
        child_q8(a.child, a.n_items, a.k, a.reps, a.q8)
        return 0
    if a.child and a.diversify:
        child_diversify(a.n_items, a.k, a.reps)
        return 0
    if a.shards_ivf < 0 or (a.shards_ivf and (not a.shards or not 1 <= a.k <= 128)):
        raise SystemExit("--shards-ivf takes 0 (off) or a number of lists per shard, goes with --shards and takes --k in 1..128")
    if a.child and a.shards and a.shards_ivf:
        child_shards_ivf(a.child, a.n_items, a.k, a.reps, a.shards, a.shards_ivf)
        return 0
    if a.child and a.shards:
        child_shards(a.child, a.n_items, a.k, a.reps, a.shards)
        return 0
    if a.child and a.ivf:
        child_ivf(a.child, a.n_items, a.k, a.reps, a.ivf)
        return 0
    if a.child:
        child(a.child, a.n_items, a.k, a.reps, a.exclude, a.group, a.tags, a.after, a.deep, a.bias)
        return 0
    for name in ["serving"] if a.diversify else a.shapes.split(","):
        if name not in SHAPES:
            raise SystemExit(f"unknown shape {name}")
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--reps", str(a.reps),
                                 "--n-items", str(a.n_items), "--k", str(a.k), "--exclude", str(a.exclude),
                                 "--group", str(a.group), "--tags", str(a.tags), "--deep", str(a.deep), "--shards", str(a.shards),
                                 "--ivf", str(a.ivf), "--q8", str(a.q8), "--ivf-filt", str(a.ivf_filt),
                                 "--ivf-deep", str(a.ivf_deep), "--ivf-heads", str(a.ivf_heads), "--ivf-q8", str(a.ivf_q8),
                                 "--shards-ivf", str(a.shards_ivf), "--baseline-lib", a.baseline_lib]
                                + (["--after"] if a.after else []) + (["--bias"] if a.bias else [])
                                + (["--diversify"] if a.diversify else []),
                                timeout=a.step_timeout).returncode
        except subprocess.TimeoutExpired:
            print(json.dumps({"shape": name, "error": f"no result within {a.step_timeout} s"}), flush=True)
            return 1
        if rc != 0:  # a failed GPU step ends the run: nothing more is started on the device
            print(json.dumps({"shape": name, "error": f"exit status {rc}"}), flush=True)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
