"""Ranking-stage benchmark: RankerModelWrapper.rank against the same stage written in torch, on the same
device, model, store and candidate lists.

    python tools/bench_rank.py [--q 256] [--m 1024] [--k 100] [--n-items 2000000] [--reps 20] [--small]

The model is the C4 ranker config (128 dense, 64 categorical x 1M rows, MLP [1024, 512] -> 1) with the
split n_user_dense = 32, n_user_categorical = 16 (--small: the reduced config of the tests, for a quick
check of the tool).  The lists are random store ids with 5 % pads.  The run is a child process of its
own (checked exit status, time limit).  One JSON line:
  rank_ms / torch_ms      median device time of one call (HIP events) with min / max; the two arms
                          alternate inside one loop.  torch arm: rows_of, index + where + cat for the batch,
                          the same forward in the same chunks, torch.sort of the masked logits (stable,
                          descending) and gathers
  rank_over_torch (_hi)   on the medians, and the worst pairing (rank max / torch min): faster only if < 1
  same_ids, same_logits   the two arms' outputs agree (ids everywhere; logits bit for bit where a slot is held)
  assemble_ms, sort_ms    the two new kernels' launches inside rank() (the library's live timer, summed over
                          the chunks of one call, median of 5 calls), kernels_share their part of rank_ms
  assemble_tbps, sort_tbps  their algorithmic bytes (the batch read once and written once, plus the rows;
                          logits and rows in, three lists out) over those times
  copy_tbps               torch copy_ of 1 GiB f32, read + write, in this process: the HBM copy rate that
                          tools/bw_probe.py reports
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


def torch_rank(m, users, ids, store, k, max_rows):
    """The stage in torch: what a user of the project writes without rank()."""
    import torch
    Q, M = ids.shape
    step = max(1, max_rows // M)
    out_ids, out_logits, out_src = [], [], []
    with torch.no_grad():
        for q0 in range(0, Q, step):
            q1 = min(Q, q0 + step)
            n = q1 - q0
            rows = store.rows_of(ids[q0:q1]).long()
            ok = (rows >= 0)[..., None]
            idx = rows.clamp(min=0)
            dense = torch.cat([users["dense"][q0:q1, None, :].expand(n, M, -1),
                               torch.where(ok, store.dense[idx], torch.zeros((), device=ids.device))], dim=-1)
            cat = torch.cat([users["categorical"][q0:q1, None, :].expand(n, M, -1),
                             torch.where(ok, store.categorical[idx], torch.zeros((), dtype=torch.int64, device=ids.device))],
                            dim=-1)
            logits = m.forward({"dense": dense.reshape(n * M, -1), "categorical": cat.reshape(n * M, -1)})["logits"]
            logits = logits.reshape(n, M).float()
            held = (rows >= 0) & ~torch.isnan(logits)
            key = torch.where(held, logits, torch.full_like(logits, float("-inf")))
            # (logit descending, row ascending, position ascending): two stable sorts
            o1 = rows.argsort(dim=1, stable=True)
            o2 = key.gather(1, o1).argsort(dim=1, descending=True, stable=True)
            src = o1.gather(1, o2)[:, :k]
            h = held.gather(1, src)
            out_ids.append(torch.where(h, ids[q0:q1].gather(1, src), torch.zeros_like(src)))
            out_logits.append(torch.where(h, logits.gather(1, src), torch.full((), float("-inf"), device=ids.device)))
            out_src.append(torch.where(h, src, torch.full_like(src, -1)).to(torch.int32))
    return torch.cat(out_ids), torch.cat(out_logits), torch.cat(out_src)


def child(Q: int, M: int, k: int, N: int, reps: int, small: bool) -> None:
    import torch
    from recommendations_amd import _lib
    from recommendations_amd.models.ranker.config import ranker_config
    from recommendations_amd.models.ranker.serving import ItemFeatureStore
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    if small:
        cfg = ranker_config(n_dense=8, n_cat=4, cat_vocab=1000, gate_sizes=(64, 32), emb_dim=16, n_user_dense=3,
                            n_user_categorical=1)
    else:
        cfg = ranker_config(n_user_dense=32, n_user_categorical=16)
    with torch.device(dev):
        m = cfg.get_builder().build()
    du, fu = cfg.n_user_dense, cfg.n_user_categorical
    di, fi = cfg.n_dense - du, cfg.n_categorical - fu
    g = torch.Generator(device=dev).manual_seed(1)
    store = ItemFeatureStore(torch.arange(1, N + 1, dtype=torch.int64, device=dev) * 3,
                             torch.randn((N, di), generator=g, device=dev),
                             torch.randint(-(2 ** 62), 2 ** 62, (N, fi), generator=g, device=dev))
    users = {"dense": torch.randn((Q, du), generator=g, device=dev),
             "categorical": torch.randint(-(2 ** 62), 2 ** 62, (Q, fu), generator=g, device=dev)}
    ids = store.ids[torch.randint(0, N, (Q, M), generator=g, device=dev)]
    ids = torch.where(torch.rand((Q, M), generator=g, device=dev) < 0.05, torch.zeros_like(ids), ids).contiguous()
    max_rows = 65536

    def rank():
        return m.rank(users, ids, store, k, max_rows=max_rows)

    def base():
        return torch_rank(m, users, ids, store, k, max_rows)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    arms = [("rank", rank, []), ("torch", base, [])]
    for _ in range(2):
        for _, fn, _ in arms:
            fn()
    torch.cuda.synchronize()
    for _ in range(reps):
        for _, fn, times in arms:
            times.append(timed(fn))
    out = {"Q": Q, "M": M, "k": k, "N": N, "reps": reps, "max_rows": max_rows, "chunks": -(-Q // max(1, max_rows // M)),
           "split": {"n_user_dense": du, "n_user_categorical": fu, "n_item_dense": di, "n_item_categorical": fi}}
    for key, _, times in arms:
        out.update({f"{key}_ms": round(statistics.median(times), 4), f"{key}_min_ms": round(min(times), 4),
                    f"{key}_max_ms": round(max(times), 4)})
    out["rank_over_torch"] = round(out["rank_ms"] / out["torch_ms"], 4)
    out["rank_over_torch_hi"] = round(out["rank_max_ms"] / out["torch_min_ms"], 4)
    a, b = rank(), base()
    held = a[2] >= 0
    out["same_ids"] = bool(torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]))
    out["same_logits"] = bool(torch.equal(a[1][held].view(torch.int32), b[1][held].view(torch.int32)))
    # the two kernels inside rank(): the library's live timer around their launches, per call
    per = {"rank_assemble_k": [], "rank_sort_k": []}
    nbytes = {}
    for _ in range(5):
        _lib.TIMER = _lib.KernelTimer(only=set(per))
        rank()
        s = _lib.TIMER.summary()
        _lib.TIMER = None
        for key in per:
            per[key].append(s[key]["ms"])
            nbytes[key] = s[key]["bytes"]
    am, sm = statistics.median(per["rank_assemble_k"]), statistics.median(per["rank_sort_k"])
    out.update({"assemble_ms": round(am, 4), "sort_ms": round(sm, 4), "kernels_share": round((am + sm) / out["rank_ms"], 4),
                "assemble_bytes": nbytes["rank_assemble_k"], "sort_bytes": nbytes["rank_sort_k"],
                "assemble_tbps": round(nbytes["rank_assemble_k"] / am / 1e9, 3),
                "sort_tbps": round(nbytes["rank_sort_k"] / sm / 1e9, 3)})
    n = 1 << 28
    x, y = torch.empty(n, dtype=torch.float32, device=dev).normal_(), torch.empty(n, dtype=torch.float32, device=dev)
    y.copy_(x)
    t = statistics.median([timed(lambda: y.copy_(x)) for _ in range(10)])
    out["copy_tbps"] = round(2 * n * 4 / t / 1e9, 3)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--q", type=int, default=256)
    ap.add_argument("--m", type=int, default=1024)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--n-items", type=int, default=2_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        child(a.q, a.m, a.k, a.n_items, a.reps, a.small)
        return
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--q", str(a.q), "--m", str(a.m), "--k", str(a.k),
           "--n-items", str(a.n_items), "--reps", str(a.reps)] + (["--small"] if a.small else [])
    rc = subprocess.run(cmd, timeout=500).returncode
    if rc != 0:
        sys.exit(f"bench_rank: the run failed with exit status {rc}")


if __name__ == "__main__":
    main()
