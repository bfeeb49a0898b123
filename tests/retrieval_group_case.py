"""The checker of the multi-head retrieval tests (test_retrieval_group_host.py pins it on the
CPU, test_gpu_retrieval_group.py holds the kernels to it): fp64 per-head scores of the bf16
operands, the maximum over a user's heads, -inf at the user's excluded rows, numpy.lexsort on
(row, -score) for the order (score descending, row ascending), and the rank as the strict count
over the non-excluded rows other than the target.  host_merge is what a caller without the
grouped kernel would do with G per-head top-k lists."""
import numpy as np

from retrieval_exclude_case import valid_rows


def group_checker(q_bf, items_bf, k, excl=None, trow=None):
    """q_bf [U, G, 128], items_bf [N, 128]: the bf16 operands; excl [U, X] integers or None (any
    order, entries outside [0, N) ignored); trow [U] or None.  Returns the fp64 per-head scores
    sg [U, G, N], their maximum s [U, N], the same with -inf at excluded rows, the expected
    (scores f32 [U, k], rows int32 [U, k]), rank int32 [U] and target_score f32 [U] (or None)."""
    U, G, D = q_bf.shape
    sg = (q_bf.double().reshape(U * G, D) @ items_bf.double().T).numpy().reshape(U, G, -1)
    s = sg.max(axis=1)
    N = s.shape[1]
    masked = s.copy()
    if excl is not None:
        for u in range(U):
            masked[u, valid_rows(excl[u], N)] = -np.inf
    rows = np.full((U, k), -1, dtype=np.int32)
    sc = np.full((U, k), -np.inf, dtype=np.float32)
    ar = np.arange(N)
    for u in range(U):
        order = np.lexsort((ar, -masked[u]))
        order = order[masked[u, order] > -np.inf][:k]
        rows[u, :len(order)] = order
        sc[u, :len(order)] = s[u, order].astype(np.float32)
    rank = tscore = None
    if trow is not None:
        rank = np.full(U, -1, dtype=np.int32)
        tscore = np.full(U, -np.inf, dtype=np.float32)
        for u in range(U):
            t = int(trow[u])
            if 0 <= t < N:  # strict, so the target never counts itself; nor does an excluded row (-inf)
                rank[u] = int((masked[u] > s[u, t]).sum())
                tscore[u] = np.float32(s[u, t])
    return sg, s, masked, sc, rows, rank, tscore


def host_merge(lists, k):
    """lists: G pairs (scores [U, k'], rows [U, k']), one per head, empty slots as row -1.  Per
    row the maximum score over the lists, then the k best by (score descending, row ascending):
    (scores f32 [U, k], rows int32 [U, k]) with -inf / -1 in empty slots."""
    U = lists[0][0].shape[0]
    sc = np.full((U, k), -np.inf, dtype=np.float32)
    rows = np.full((U, k), -1, dtype=np.int32)
    for u in range(U):
        best = {}
        for scores_g, rows_g in lists:
            for v, r in zip(scores_g[u].tolist(), rows_g[u].tolist()):
                if r >= 0 and (r not in best or v > best[r]):
                    best[r] = v
        order = sorted(best.items(), key=lambda it: (-it[1], it[0]))[:k]
        for i, (r, v) in enumerate(order):
            rows[u, i], sc[u, i] = r, np.float32(v)
    return sc, rows
