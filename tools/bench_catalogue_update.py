#!/usr/bin/env python
"""Catalogue updates against the rebuild they replace, on the clustered catalogue of DESIGN.md section 16.

    python tools/bench_catalogue_update.py [--n-items 2000000] [--lists 4096] [--fractions 0.001,0.1]
                                           [--reps 10] [--warmup 3] [--step-timeout 420]

The catalogue: N unit rows around 4,096 random unit centres (tools/bench_retrieval.py --ivf draws the
same), random distinct int64 ids, tags and a bias, clustered into L lists by ItemCatalogue.cluster.  An
update of fraction f upserts f N rows, half of them replacements of random items and half new ids, drawn
like the catalogue, and removes f N other random items.

Three things are timed per fraction, in one process, the two calls alternating inside the loop:
  kernel    the launches of lthm_catalogue_update alone (the library's live timer: HIP events around
            the C call inside ClusteredItemCatalogue.update)
  update    the whole ClusteredItemCatalogue.update call, its one host read included (host clock around a
            call that ends in a device synchronise)
  rebuild   the definition on the public API there was before: drop the removed and replaced rows of the
            flat catalogue, append the upsert rows, sort by id, give the upsert rows their nearest list
            (K.retrieve_topk, k = 1) while the others keep theirs, ClusteredItemCatalogue.from_assignment
The results of the two are compared tensor by tensor before anything is timed.  Reported beside the
medians: update / rebuild, kernel / the copy floor 2 N' bytes-per-row / 4.8 TB/s (the copy rate DESIGN.md
section 9 measured), and the peak device memory of each path above what the catalogue and the arguments hold.

Every fraction runs in a process of its own under --step-timeout; a step that fails or runs out of time
ends the run, and nothing more is started on the device.  One JSON line per fraction."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

COPY_RATE = 4.8e12  # bytes / s, DESIGN.md section 9


def child(N: int, L: int, frac: float, reps: int, warmup: int) -> None:
    import statistics
    import time
    import torch
    from recommendations_amd import _lib
    from recommendations_amd import kernels as K
    from recommendations_amd.models.lthm.sequence.retrieval import ClusteredItemCatalogue, ItemCatalogue
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    C, sigma = 4096, 0.7 / 128 ** 0.5
    centres = torch.nn.functional.normalize(torch.randn((C, 128), generator=g, device=dev), dim=-1)

    def draw(n):
        out = torch.empty((n, 128), dtype=torch.bfloat16, device=dev)
        for lo in range(0, n, 1 << 18):
            m = min(1 << 18, n - lo)
            x = centres[torch.randint(0, C, (m,), generator=g, device=dev)] + sigma * torch.randn((m, 128), generator=g, device=dev)
            out[lo:lo + m] = torch.nn.functional.normalize(x, dim=-1).to(torch.bfloat16)
        return out

    n_up = max(2, int(round(frac * N)))
    n_new, n_rep, n_rm = n_up // 2, n_up - n_up // 2, n_up
    pool = torch.randint(-(2 ** 63), 2 ** 63 - 1, (N + n_new + (N >> 6) + 64,), dtype=torch.int64, generator=g, device=dev)
    pool = torch.unique(pool[pool != 0])
    pool = pool[torch.randperm(pool.numel(), generator=g, device=dev)]
    assert pool.numel() >= N + n_new
    ids, new_ids = torch.sort(pool[:N])[0], pool[N:N + n_new]
    cols = lambda n: (torch.randint(-(2 ** 31), 2 ** 31 - 1, (n,), generator=g, device=dev).to(torch.int32),
                      torch.randn(n, generator=g, device=dev))
    flat = ItemCatalogue(ids, draw(N), *cols(N))
    cl = flat.cluster(L, iters=5, seed=0, sample=min(N, 1 << 18))
    # the list of every flat row, which a rebuild has to keep
    assign = torch.repeat_interleave(torch.arange(L, device=dev), cl.list_lengths())[cl.rows_of(flat.ids).long()]
    picked = torch.randperm(N, generator=g, device=dev)[:n_rep + n_rm]
    upsert = ItemCatalogue.from_embeddings(torch.cat([ids[picked[:n_rep]], new_ids]), draw(n_up), *cols(n_up))
    remove_ids = ids[picked[n_rep:]].contiguous()
    lens = cl.list_lengths()

    def update():
        return cl.update(upsert, remove_ids)

    def rebuild():
        keep = ~(torch.isin(flat.ids, remove_ids) | torch.isin(flat.ids, upsert.ids))
        up_assign = K.retrieve_topk(upsert.emb, cl.centroids, 1, normalize_q=False)[1][:, 0].long()
        all_ids = torch.cat([flat.ids[keep], upsert.ids])
        order = torch.argsort(all_ids)
        pick = lambda a, b: torch.cat([a[keep], b])[order]
        flat2 = ItemCatalogue(all_ids[order], pick(flat.emb, upsert.emb), pick(flat.tags, upsert.tags),
                              pick(flat.bias, upsert.bias))
        return ClusteredItemCatalogue.from_assignment(flat2, cl.centroids, pick(assign, up_assign))

    got, want = update(), rebuild()
    for name in ("row_ids", "emb", "list_off", "tags", "bias", "_ids", "_order"):
        a, b = getattr(got, name), getattr(want, name)
        assert torch.equal(a.view(torch.int16) if a.dtype == torch.bfloat16 else a, b.view(torch.int16) if b.dtype == torch.bfloat16 else b), name
    n_out = len(got)
    del got, want

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        held = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        return (torch.cuda.max_memory_allocated() - held) / 2 ** 20

    for _ in range(warmup):
        update()
        rebuild()
    t_up, t_re = [], []
    for _ in range(reps):  # alternating, so that drift hits both alike
        t_up.append(timed(update))
        t_re.append(timed(rebuild))
    _lib.TIMER = _lib.KernelTimer(only={"cat_upd_merge_k"})
    for _ in range(reps):
        update()
    rec = _lib.TIMER.summary()["cat_upd_merge_k"]
    _lib.TIMER = None
    kernel_ms = rec["ms"] / rec["calls"]
    row_bytes = 128 * 2 + 8 + 4 + 4
    floor_ms = 2.0 * n_out * row_bytes / COPY_RATE * 1e3
    med = statistics.median
    print(json.dumps({
        "N": N, "L": L, "fraction": frac, "upserts": n_up, "replacements": n_rep, "removes": n_rm, "N_out": n_out,
        "list_len_min": int(lens.min()), "list_len_median": int(lens.median()), "list_len_max": int(lens.max()),
        "device": torch.cuda.get_device_name(0), "reps": reps, "warmup": warmup,
        "kernel_ms": round(kernel_ms, 4), "update_ms": round(med(t_up), 3), "update_ms_min": round(min(t_up), 3),
        "update_ms_max": round(max(t_up), 3), "rebuild_ms": round(med(t_re), 3), "rebuild_ms_min": round(min(t_re), 3),
        "rebuild_ms_max": round(max(t_re), 3), "update_over_rebuild": round(med(t_up) / med(t_re), 4),
        "copy_floor_ms": round(floor_ms, 4), "kernel_over_floor": round(kernel_ms / floor_ms, 3),
        "kernel_TBps": round(2.0 * n_out * row_bytes / (kernel_ms * 1e-3) / 1e12, 3),
        "update_peak_MiB": round(peak(update), 1), "rebuild_peak_MiB": round(peak(rebuild), 1)}), flush=True)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n-items", type=int, default=2_000_000)
    ap.add_argument("--lists", type=int, default=4096)
    ap.add_argument("--fractions", default="0.001,0.1")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=420)
    ap.add_argument("--child", type=float, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child is not None:
        child(a.n_items, a.lists, a.child, a.reps, a.warmup)
        return 0
    for frac in a.fractions.split(","):
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", frac, "--n-items", str(a.n_items),
                                 "--lists", str(a.lists), "--reps", str(a.reps), "--warmup", str(a.warmup)],
                                timeout=a.step_timeout).returncode
        except subprocess.TimeoutExpired:
            print(json.dumps({"fraction": frac, "error": f"no result within {a.step_timeout} s"}), flush=True)
            return 1
        if rc != 0:  # a failed GPU step ends the run: nothing more is started on the device
            print(json.dumps({"fraction": frac, "error": f"exit status {rc}"}), flush=True)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
