"""The checker of the tag-filter retrieval tests (test_retrieval_tags_host.py pins it on the CPU,
test_gpu_retrieval_tags.py holds the kernels to it): fp64 scores of the bf16 operands, the
maximum over a user's heads, -inf at the rows the user's filter makes ineligible and at the
user's excluded rows, numpy.lexsort on (row, -score) for the order (score descending, row
ascending), and the rank as the strict count over the eligible, non-excluded rows other than the
target.  The target itself is never filtered: its score is the plain (best-over-heads) dot."""
import numpy as np

from retrieval_exclude_case import valid_rows


def bits32(x):
    """Integers (int32 bit patterns or values in 0..2^32-1) as their 32 bits, in int64."""
    return np.asarray(x).astype(np.int64) & 0xFFFFFFFF


def eligible(tags, filt):
    """tags [N], filt [Q, 3] = (all, any, none) -> bool [Q, N]:
    (tags & all) == all  and  (any == 0 or tags & any != 0)  and  tags & none == 0."""
    t = bits32(tags)[None, :]
    f = bits32(filt)
    fa, fy, fn = f[:, 0:1], f[:, 1:2], f[:, 2:3]
    return ((t & fa) == fa) & ((fy == 0) | ((t & fy) != 0)) & ((t & fn) == 0)


def tags_checker(q_bf, items_bf, k, tags=None, filt=None, excl=None, trow=None):
    """q_bf [Q, 128] or [U, G, 128] and items_bf [N, 128]: the bf16 operands; tags [N] and filt
    [U, 3] integers, or both None; excl [U, X] integers or None (any order, entries outside
    [0, N) ignored); trow [U] or None.  Returns the fp64 best-over-heads scores s [U, N], the
    same with -inf at ineligible and excluded rows, the expected (scores f32 [U, k], rows int32
    [U, k]), rank int32 [U] and target_score f32 [U] (or None)."""
    if q_bf.dim() == 2:
        q_bf = q_bf[:, None, :]
    U, G, D = q_bf.shape
    sg = (q_bf.double().reshape(U * G, D) @ items_bf.double().T).numpy().reshape(U, G, -1)
    s = sg.max(axis=1)
    N = s.shape[1]
    masked = s.copy()
    if tags is not None:
        masked[~eligible(tags, filt)] = -np.inf
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
            if 0 <= t < N:  # strict: the target never counts itself, nor does a row at -inf
                rank[u] = int((np.delete(masked[u], t) > s[u, t]).sum())
                tscore[u] = np.float32(s[u, t])
    return s, masked, sc, rows, rank, tscore
