"""The checker of the exclusion tests (test_retrieval_exclude_host.py pins it on the CPU,
test_gpu_retrieval_exclude.py holds the kernels to it): fp64 scores of the bf16 operands with
-inf at a query's excluded rows, numpy.lexsort on (row, -score) for the order (score
descending, row ascending), and the rank as the strict count over the non-excluded rows other
than the target."""
import numpy as np


def valid_rows(lst, N):
    """The entries of one exclusion list that name a catalogue row."""
    lst = np.asarray(lst, dtype=np.int64)
    return np.unique(lst[(lst >= 0) & (lst < N)])


def excl_checker(q_bf, items_bf, k, excl, trow=None):
    """q_bf [Q, 128], items_bf [N, 128]: the bf16 operands; excl [Q, X] integers (any order,
    entries outside [0, N) ignored); trow [Q] or None.  Returns the fp64 scores s [Q, N], the
    same with -inf at excluded rows, the expected (scores f32 [Q, k], rows int32 [Q, k]) and
    rank int32 [Q] (or None)."""
    s = (q_bf.double() @ items_bf.double().T).numpy()
    Q, N = s.shape
    masked = s.copy()
    for i in range(Q):
        masked[i, valid_rows(excl[i], N)] = -np.inf
    rows = np.full((Q, k), -1, dtype=np.int32)
    sc = np.full((Q, k), -np.inf, dtype=np.float32)
    ar = np.arange(N)
    for i in range(Q):
        order = np.lexsort((ar, -masked[i]))
        order = order[masked[i, order] > -np.inf][:k]
        rows[i, :len(order)] = order
        sc[i, :len(order)] = s[i, order].astype(np.float32)
    rank = None
    if trow is not None:
        rank = np.full(Q, -1, dtype=np.int32)
        for i in range(Q):
            t = int(trow[i])
            if 0 <= t < N:  # strict, so the target never counts itself; nor does an excluded row (-inf)
                rank[i] = int((masked[i] > s[i, t]).sum())
    return s, masked, sc, rows, rank
